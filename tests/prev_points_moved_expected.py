"""numpy restatement of rt_hip_prev_points_moved (include/rt_hip.h): rt_hip_prev_points' clauses, and for a hit on a sphere that
moved, s = r' / r and out_k = c'_k + (point_k - c_k) * s -- fp64, unfused, in that order.  tests/test_sphere_update_cpu.py pins it
against a scalar Python statement; tests/test_gpu_prev_points_moved.py compares the kernel with it bit for bit."""
import numpy as np

QNAN = np.uint64(0x7FF8000000000000)
NO_PRIM = 0xFFFFFFFF


def prev_points_moved(hits, positions, spheres_prev, spheres_cur):
    """hits: numpy arrays status, prim, object (n), bary (n, 2), point (n, 3); positions: (n_triangles, 3, 3) or None;
    spheres_prev / spheres_cur: (n_spheres, 4), or both None (no sphere moved: a sphere hit keeps its point's bits) -> (n, 3)"""
    status = np.asarray(hits["status"]).view(np.uint32).ravel()
    prim = np.asarray(hits["prim"]).view(np.uint32).ravel()
    obj = np.asarray(hits["object"]).view(np.uint32).ravel()
    bary = np.asarray(hits["bary"], dtype=np.float64).reshape(-1, 2)
    point = np.ascontiguousarray(hits["point"], dtype=np.float64).reshape(-1, 3)
    n = len(status)
    out = np.full((n, 3), 0.0)
    out.view(np.uint64)[:] = QNAN
    hit = status == 1
    on_sphere = hit & (prim == NO_PRIM)
    if spheres_prev is None:
        assert spheres_cur is None
        out.view(np.uint64)[on_sphere] = point.view(np.uint64)[on_sphere]
    else:
        was = np.asarray(spheres_prev, dtype=np.float64).reshape(-1, 4)
        now = np.asarray(spheres_cur, dtype=np.float64).reshape(-1, 4)
        m = on_sphere & (obj.astype(np.uint64) < len(was))
        k = obj[m].astype(np.int64)
        with np.errstate(all="ignore"):
            s = was[k, 3] / now[k, 3]
            out[m] = was[k, :3] + (point[m] - now[k, :3]) * s[:, None]
    pos = np.zeros((0, 3, 3)) if positions is None else np.asarray(positions, dtype=np.float64).reshape(-1, 3, 3)
    m = hit & (prim != NO_PRIM) & (prim.astype(np.uint64) < len(pos))
    t = pos[prim[m].astype(np.int64)]
    with np.errstate(all="ignore"):
        u, v = bary[m, 0:1], bary[m, 1:2]
        w0 = (1.0 - u) - v
        out[m] = (t[:, 0] * w0 + t[:, 1] * u) + t[:, 2] * v
    return out


def prev_points_moved_scalar(hits, positions, spheres_prev, spheres_cur):
    """the same, entry by entry in Python floats (IEEE doubles, one rounding per operation)"""
    n = len(hits["status"])
    out = np.zeros((n, 3))
    for i in range(n):
        res = None
        if int(hits["status"][i]) & 0xFFFFFFFF == 1:
            prim, obj = int(hits["prim"][i]) & 0xFFFFFFFF, int(hits["object"][i]) & 0xFFFFFFFF
            if prim == NO_PRIM:
                if spheres_prev is None:
                    out.view(np.uint64)[i] = np.ascontiguousarray(hits["point"][i], dtype=np.float64).view(np.uint64)
                    continue
                if obj < len(spheres_prev):
                    was, now = [float(x) for x in spheres_prev[obj]], [float(x) for x in spheres_cur[obj]]
                    with np.errstate(all="ignore"):
                        s = float(np.float64(was[3]) / np.float64(now[3]))   # (Python raises on a division by zero; numpy's scalar does not)
                        res = [float(np.float64(was[k]) + (np.float64(float(hits["point"][i][k])) - np.float64(now[k])) * np.float64(s))
                               for k in range(3)]
            elif positions is not None and prim < len(positions):
                u, v = float(hits["bary"][i][0]), float(hits["bary"][i][1])
                w0 = (1.0 - u) - v
                t = positions[prim]
                with np.errstate(all="ignore"):
                    res = [float((np.float64(t[0][k]) * w0 + np.float64(t[1][k]) * u) + np.float64(t[2][k]) * v) for k in range(3)]
        if res is None:
            out.view(np.uint64)[i] = QNAN
        else:
            out[i] = res
    return out


def same(got, want):
    """bit for bit, but a NaN the arithmetic itself made compares as NaN (its sign and payload are the machine's)"""
    g, w = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return g.shape == w.shape and bool(((g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))).all())


def planted(n_spheres, n_triangles, seed=5):
    """entries that no query returns: status 0 and 2, object == n_spheres, object == 0xFFFFFFFF with status 1, a sphere whose
    radius did not change (s = 1), a radius ratio that overflows to inf (1e200 / 1e-200), a prim out of range -> (hits, spheres_prev,
    spheres_cur) with n_spheres >= 4"""
    rng = np.random.default_rng(seed)
    rows = [(0, NO_PRIM, 1), (2, NO_PRIM, 1), (1, NO_PRIM, n_spheres), (1, NO_PRIM, 0xFFFFFFFF), (1, NO_PRIM, 2), (1, NO_PRIM, 3),
            (1, n_triangles, 0), (1, 0 if n_triangles else 7, 0), (1, NO_PRIM, 0), (0, 0, 0)]
    n = len(rows)
    hits = dict(status=np.array([r[0] for r in rows], dtype=np.uint32), prim=np.array([r[1] for r in rows], dtype=np.uint32),
                object=np.array([r[2] for r in rows], dtype=np.uint32), bary=rng.uniform(0, 0.5, (n, 2)), point=rng.uniform(-9, 9, (n, 3)))
    prev = np.concatenate([rng.uniform(-5, 5, (n_spheres, 3)), rng.uniform(0.5, 3, (n_spheres, 1))], axis=1)
    cur = prev + rng.uniform(-0.5, 0.5, prev.shape) * np.array([1, 1, 1, 0.2])
    cur[2, 3] = prev[2, 3]                    # r = r': s = 1
    prev[3, 3], cur[3, 3] = 1e200, 1e-200     # s = inf
    return hits, prev, cur
