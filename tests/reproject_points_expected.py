"""The two contracts of reprojection across vertex updates (include/rt_hip.h, rt_hip_prev_points and rt_hip_reproject_points)
restated in numpy, in the manner of tests/reproject_expected.py, whose helpers this file imports: vectorised forms, a scalar
line-by-line form of each, and the edge inputs both are compared on, and the GPU against them.  fp64 +, -, * in the written order
(numpy's float64 arithmetic is IEEE and never fuses)."""
import math

import numpy as np

import reproject_expected as RE
from reproject_expected import QNAN, _cross, _div, _dot, _scross, _sdot, _sqrt, cam_array, f32

QNAN64_BITS = np.uint64(0x7FF8000000000000)
NO_PRIM = 0xFFFFFFFF
DENORM64 = 5e-324


# ---- rt_hip_prev_points ----------------------------------------------------------------------------------------------------------

def prev_points(status, prim, bary, point, positions):
    """status, prim uint32 [n]; bary float64 [n, 2]; point float64 [n, 3]; positions float64 [n_tri, 3, 3] or None
    -> float64 [n, 3]; the sphere branch copies bits"""
    status, prim = np.asarray(status, np.uint32).reshape(-1), np.asarray(prim, np.uint32).reshape(-1)
    n = len(status)
    bary, point = np.asarray(bary, np.float64).reshape(n, 2), np.ascontiguousarray(point, np.float64).reshape(n, 3)
    pos = np.zeros((0, 3, 3)) if positions is None else np.asarray(positions, np.float64).reshape(-1, 3, 3)
    out = np.full((n, 3), QNAN64_BITS, np.uint64)
    hit = status == 1
    sphere = hit & (prim == NO_PRIM)
    out[sphere] = point.view(np.uint64)[sphere]
    tri = hit & (prim < len(pos))
    if tri.any():
        with np.errstate(all="ignore"):
            t = pos[prim[tri]]
            u, v = bary[tri, 0:1], bary[tri, 1:2]
            w0 = (1.0 - u) - v
            out[tri] = ((t[:, 0] * w0 + t[:, 1] * u) + t[:, 2] * v).view(np.uint64)
    return out.view(np.float64)


def scalar_prev_points(status, prim, bary, point, positions):
    n = len(status)
    n_tri = 0 if positions is None else len(positions)
    out = np.zeros((n, 3), np.uint64)
    pbits = np.ascontiguousarray(point, np.float64).reshape(n, 3).view(np.uint64)
    for i in range(n):
        out[i] = QNAN64_BITS
        if int(status[i]) != 1:
            continue
        k = int(prim[i])
        if k == NO_PRIM:
            out[i] = pbits[i]
        elif k < n_tri:
            u, v = float(bary[i][0]), float(bary[i][1])
            w0 = (1.0 - u) - v
            a, b, c = [[float(t) for t in positions[k][j]] for j in range(3)]
            with np.errstate(all="ignore"):
                vals = [(np.float64(a[j]) * w0 + np.float64(b[j]) * u) + np.float64(c[j]) * v for j in range(3)]
            out[i] = np.array(vals, np.float64).view(np.uint64)
    return out.view(np.float64)


def same_bits64(got, exp):
    g, e = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(exp, np.float64)
    return g.shape == e.shape and bool((g.view(np.uint64) == e.view(np.uint64)).all())


def same_points(got, exp, status, prim, n_tri):
    """bit for bit, but for the NaNs the triangle branch's arithmetic makes (inf - inf, 0 * inf, a NaN operand): IEEE 754 leaves
    their sign and payload to the machine, so there NaN equals NaN as in RE.same_floats.  The quiet NaNs the contract names and
    the words the sphere branch copies are compared as bits"""
    g, e = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(exp, np.float64)
    if g.shape != e.shape:
        return False
    tri = ((np.asarray(status, np.uint32) == 1) & (np.asarray(prim, np.uint32) < n_tri)).reshape(-1, 1)
    return bool(((g.view(np.uint64) == e.view(np.uint64)) | (tri & np.isnan(g) & np.isnan(e))).all())


BARY_VALUES = (0.0, 1.0, -0.0, 0.5, np.nan, np.inf, 1e300, DENORM64)
STATUS_VALUES = (0, 1, 2, 3)


def nan_payload_points(n, rng):
    """point words: ordinary values with NaNs of other payloads (signalling ones among them), infinities and -0.0 mixed in"""
    p = rng.normal(size=(n, 3)) * 10.0
    bits = p.view(np.uint64)
    special = np.array([0x7FF8000000000123, 0x7FF0000000000001, 0xFFF8DEADBEEF0001, 0x7FF0000000000000, 0x8000000000000000,
                        0xFFFFFFFFFFFFFFFF], np.uint64)
    at = rng.random((n, 3)) < 0.3
    bits[at] = special[rng.integers(0, len(special), int(at.sum()))]
    return p


def prim_values(n_tri):
    return sorted({0, max(n_tri - 1, 0), n_tri, 0xFFFFFFFE, NO_PRIM})


def edge_hits(n, n_tri, seed):
    """-> status, prim, bary, point: the first entries run through every (status, prim, u, v) of the value lists in turn (the
    whole product when n allows), the rest are drawn from them at random with ordinary barycentrics mixed in"""
    rng = np.random.default_rng(seed)
    prims = prim_values(n_tri)
    grid = [(s, p, u, v) for s in STATUS_VALUES for p in prims for u in BARY_VALUES for v in BARY_VALUES]
    status, prim, bary = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, 2))
    order = rng.permutation(len(grid))
    for i in range(n):
        if i < len(grid):
            s, p, u, v = grid[order[i]] if n < len(grid) else grid[i]
        else:
            s, p = int(rng.choice([0, 1, 1, 1, 2, 3])), int(rng.choice(prims + [int(rng.integers(0, max(n_tri, 1)))] * 3))
            u, v = (float(rng.choice(BARY_VALUES)), float(rng.choice(BARY_VALUES))) if rng.random() < 0.3 else tuple(rng.random(2) * 0.5)
        status[i], prim[i], bary[i] = s, p, (u, v)
    return status, prim, bary, nan_payload_points(n, rng)


def edge_positions(tris, seed):
    """the mesh with corners of +-1e300 planted into a third of its triangles (any bits are allowed: these are not scene vertices)"""
    rng = np.random.default_rng(seed)
    t = np.array(tris, np.float64).reshape(-1, 3, 3)
    at = rng.random(t.shape) < 0.1
    t[at] = rng.choice([1e300, -1e300], int(at.sum()))
    return t


def branch_counts(status, prim, n_tri):
    status, prim = np.asarray(status, np.uint32), np.asarray(prim, np.uint32)
    hit = status == 1
    return dict(not_hit=int((~hit).sum()), sphere=int((hit & (prim == NO_PRIM)).sum()), triangle=int((hit & (prim < n_tri)).sum()),
                other_prim=int((hit & (prim != NO_PRIM) & (prim >= n_tri)).sum()))


# ---- rt_hip_reproject_points -----------------------------------------------------------------------------------------------------

def reproject(rgb, aov, camera, hist=None, prev_points=None, max_history=32.0, depth_tol=0.05, normal_min=0.5, info=None):
    """RE.reproject with step 3 replaced by P = prev_points (float64 [H,W,3]); prev_points None: RE.reproject itself.  info as
    RE.reproject's, and nonfinite_point: pixels that passed steps 1 and 2 and ended at step 3'"""
    if prev_points is None:
        return RE.reproject(rgb, aov, camera, hist, max_history=max_history, depth_tol=depth_tol, normal_min=normal_min, info=info)
    c = np.ascontiguousarray(rgb, np.float32)
    h, w = c.shape[:2]
    out = c.copy()
    ln = np.ones((h, w), np.float32)
    motion = np.full((h, w, 2), QNAN, np.float32)
    finite = np.isfinite(c).all(axis=2)
    ln[~finite] = 0                                                          # 1.
    res = dict(rgb=out, len=ln, motion=motion)
    if hist is None:                                                         # 2.
        return res
    with np.errstate(all="ignore"):
        z = np.asarray(aov["depth"], np.float32).astype(np.float64)
        cand2 = finite & (np.asarray(aov["hits"], np.uint32) != 0) & (z > 0) & (z < np.inf)
        P = np.asarray(prev_points, np.float64).reshape(h, w, 3)             # 3'.
        cand = cand2 & np.isfinite(P).all(axis=2)
        posh, Hh, Vh, llch = cam_array(hist["camera"])                       # 4.
        D = P - posh
        R = posh - llch
        N = _cross(Vh, D)
        det = _dot(Hh, N)
        us = _dot(R, N) / det
        M = _cross(D, Hh)
        vs = _dot(R, M) / det
        k = _dot(R, _cross(Hh, Vh))
        front = ((k > 0) & (det > 0)) | ((k < 0) & (det < 0))
        fx = us * (float(w) - 1.0) - 0.5
        fy = vs * (float(h) - 1.0) - 0.5
        in_frame = (fx > -1.0) & (fx < float(w)) & (fy > -1.0) & (fy < float(h))
        ok = cand & front & in_frame
        ys, xs = np.mgrid[0:h, 0:w]
        mo = np.stack([fx - xs, fy - ys], axis=-1).astype(np.float32)
        motion[ok] = mo[ok]
        x0d, y0d = np.floor(fx), np.floor(fy)                                # 5.
        a, b = fx - x0d, fy - y0d
        x0, y0 = np.where(ok, x0d, 0.0).astype(np.int64), np.where(ok, y0d, 0.0).astype(np.int64)
        zexp = np.sqrt(_dot(D, D))
        ztol = depth_tol * zexp
        n_p = np.asarray(aov["normal"], np.float32).astype(np.float64)
        o_p = np.asarray(aov["object"], np.uint32)
        hrgb = np.ascontiguousarray(hist["rgb"], np.float32)
        hlen = np.asarray(hist["len"], np.float32).astype(np.float64)
        hn = np.asarray(hist["aov"]["normal"], np.float32).astype(np.float64)
        hz = np.asarray(hist["aov"]["depth"], np.float32).astype(np.float64)
        hh = np.asarray(hist["aov"]["hits"], np.uint32)
        ho = np.asarray(hist["aov"]["object"], np.uint32)
        W, S, A = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3))
        why = {r: np.zeros((h, w), bool) for r in RE.REASONS}
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qxc, qyc = np.where(inside, qx, xs), np.where(inside, qy, ys)
                wt = (a if i else 1.0 - a) * (b if j else 1.0 - b)
                hq = hrgb[qyc, qxc]
                lq = hlen[qyc, qxc]
                t_fin = np.isfinite(hq).all(axis=2)
                t_len = (lq >= 1.0) & (lq < np.inf)
                t_hit = hh[qyc, qxc] > 0
                t_obj = ho[qyc, qxc] == o_p
                t_nrm = _dot(n_p, hn[qyc, qxc]) >= normal_min
                t_dep = np.abs(hz[qyc, qxc] - zexp) <= ztol
                take = ok & inside & t_fin & t_len & t_hit & t_obj & t_nrm & t_dep
                W = np.where(take, W + wt, W)
                A = np.where(take[..., None], A + wt[..., None] * hq.astype(np.float64), A)
                S = np.where(take, S + wt * lq, S)
                for r, t in (("object", t_obj), ("normal", t_nrm), ("depth", t_dep), ("nonfinite_history", t_fin)):
                    why[r] |= ok & inside & ~t
        blend = ok & (W > 0)                                                 # 6.
        hc = (A / W[..., None]).astype(np.float32).astype(np.float64)
        Nn = S / W + 1.0
        Nn = np.where(Nn > max_history, max_history, Nn)
        al = 1.0 / Nn
        o = (hc + (c.astype(np.float64) - hc) * al[..., None]).astype(np.float32)
        out[blend] = o[blend]
        ln[blend] = Nn.astype(np.float32)[blend]
        capped = blend & (S / W + 1.0 > max_history)
    if info is not None:
        why["behind"] = cand & ~front
        why["out_of_frame"] = cand & front & ~in_frame
        info.update(why, candidate=cand, ok=ok, blended=blend, capped=capped, nonfinite_point=cand2 & ~cand, det_zero=cand & (det == 0))
    return res


def scalar_reproject(rgb, aov, camera, hist=None, prev_points=None, max_history=32.0, depth_tol=0.05, normal_min=0.5):
    if prev_points is None:
        return RE.scalar_reproject(rgb, aov, camera, hist, max_history=max_history, depth_tol=depth_tol, normal_min=normal_min)
    h, w = aov["depth"].shape
    out = np.zeros((h, w, 3), np.float32)
    ln = np.zeros((h, w), np.float32)
    motion = np.zeros((h, w, 2), np.float32)
    pts = np.asarray(prev_points, np.float64).reshape(h, w, 3)
    if hist is not None:
        posh, Hh, Vh, llch = [tuple(float(t) for t in r) for r in cam_array(hist["camera"])]
    inf = math.inf
    for y in range(h):
        for x in range(w):
            c = [float(rgb[y, x, k]) for k in range(3)]
            out[y, x] = rgb[y, x]
            motion[y, x] = QNAN
            # 1.
            if not all(math.isfinite(t) for t in c):
                ln[y, x] = 0.0
                continue
            ln[y, x] = 1.0
            # 2.
            zp = float(aov["depth"][y, x])
            if hist is None or int(aov["hits"][y, x]) == 0 or not (zp > 0 and zp < inf):
                continue
            # 3'.
            P = [float(t) for t in pts[y, x]]
            if not all(math.isfinite(t) for t in P):
                continue
            # 4.
            with np.errstate(all="ignore"):
                D = [float(np.float64(P[k]) - posh[k]) for k in range(3)]
                R = [posh[k] - llch[k] for k in range(3)]
                Dn = [np.float64(t) for t in D]              # (numpy scalars: products of 1e300 overflow to inf, not to an exception)
                N = _scross([np.float64(t) for t in Vh], Dn)
                det = float(_sdot(Hh, N))
                us = _div(float(_sdot(R, N)), det)
                M = _scross(Dn, [np.float64(t) for t in Hh])
                vs = _div(float(_sdot(R, M)), det)
                kk = _sdot(R, _scross(Hh, Vh))
                front = (kk > 0 and det > 0) or (kk < 0 and det < 0)
                fx = float(np.float64(us) * (w - 1.0) - 0.5)
                fy = float(np.float64(vs) * (h - 1.0) - 0.5)
                if not (front and fx > -1 and fx < w and fy > -1 and fy < h):
                    continue
                motion[y, x] = (np.float32(fx - x), np.float32(fy - y))
                # 5.
                x0, y0 = math.floor(fx), math.floor(fy)
                a, b = fx - x0, fy - y0
                zexp = _sqrt(float(_sdot(Dn, Dn)))
            W, S, A = 0.0, 0.0, [0.0, 0.0, 0.0]
            n_p = [float(t) for t in aov["normal"][y, x]]
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = x0 + i, y0 + j
                    wt = (a if i else 1.0 - a) * (b if j else 1.0 - b)
                    if qx < 0 or qx >= w or qy < 0 or qy >= h:
                        continue
                    hq = [float(t) for t in hist["rgb"][qy, qx]]
                    lq = float(hist["len"][qy, qx])
                    if not all(math.isfinite(t) for t in hq) or not (lq >= 1 and lq < inf):
                        continue
                    if not int(hist["aov"]["hits"][qy, qx]) > 0 or int(hist["aov"]["object"][qy, qx]) != int(aov["object"][y, x]):
                        continue
                    if not _sdot(n_p, [float(t) for t in hist["aov"]["normal"][qy, qx]]) >= normal_min:
                        continue
                    with np.errstate(all="ignore"):
                        if not abs(float(hist["aov"]["depth"][qy, qx]) - zexp) <= float(np.float64(depth_tol) * zexp):
                            continue
                    W += wt
                    for k in range(3):
                        A[k] += wt * hq[k]
                    S += wt * lq
            # 6.
            if not W > 0:
                continue
            Nn = _div(S, W) + 1.0
            if Nn > max_history:
                Nn = max_history
            al = _div(1.0, Nn)
            for k in range(3):
                hc = f32(_div(A[k], W))
                out[y, x, k] = np.float32(hc + (c[k] - hc) * al)
            ln[y, x] = np.float32(Nn)
    return dict(rgb=out, len=ln, motion=motion)


# ---- inputs ------------------------------------------------------------------------------------------------------------------

def step3_points(aov, camera, w, h):
    """step 3's own P = pos + d*z of rt_hip_reproject, float64 [h, w, 3]"""
    pos = cam_array(camera)[0]
    _, _, d = RE.camera_ray_dirs(camera, w, h)
    with np.errstate(all="ignore"):
        return pos + d * np.asarray(aov["depth"], np.float32).astype(np.float64)[..., None]


POINT_PLANTED = ("nan", "inf", "at_camera", "behind", "out_of_frame", "plus_1e300", "minus_1e300", "denormal", "neg_zero", "sub_pixel",
                 "pixels_away")


def _floor_point(hcam, fx, fy, w, h):
    """the point of the floor y = 0 that the history's camera sees at the continuous pixel position (fx, fy): the inverse of step 4"""
    pos, H, V, llc = hcam
    with np.errstate(all="ignore"):
        u, v = (fx + 0.5) / (w - 1.0), (fy + 0.5) / (h - 1.0)
        wv = pos - (llc + (H * u + V * v))
        d = wv * (1.0 / np.sqrt(_dot(wv, wv)))
        return pos + d * (-pos[1] / d[1])


def planted_points(w, h, kind, seed, share=0.6):
    """RE.edge_case(w, h, kind, seed) and previous points for it -> rgb, aov, cur, hist, points float64 [h, w, 3], planted:
    category -> pixel indices.  The points start as step 3's own; `share` of the pixels get the POINT_PLANTED values in turn"""
    rgb, aov, cur, hist, _ = RE.edge_case(w, h, kind, seed)
    rng = np.random.default_rng(seed + 77)
    finite_cam = lambda c: np.where(np.isfinite(c), c, 1.0)
    pts = step3_points(aov, finite_cam(cur), w, h)
    hcam = finite_cam(cam_array(hist["camera"]))
    planted = {c: [] for c in POINT_PLANTED}
    order = rng.permutation(w * h)
    for k, p in enumerate(order[: int(share * w * h)]):
        cat = POINT_PLANTED[k % len(POINT_PLANTED)]
        y, x = divmod(int(p), w)
        planted[cat].append(int(p))
        ch = int(rng.integers(0, 3))
        with np.errstate(all="ignore"):
            if cat == "nan":
                pts[y, x, ch] = np.nan
            elif cat == "inf":
                pts[y, x, ch] = [np.inf, -np.inf][k % 2]
            elif cat == "at_camera":
                pts[y, x] = cam_array(hist["camera"])[0]
            elif cat == "behind":                      # mirrored through the history's camera position
                pts[y, x] = hcam[0] - (_floor_point(hcam, x + 0.25, y + 0.25, w, h) - hcam[0])
            elif cat == "out_of_frame":
                pts[y, x] = _floor_point(hcam, [3.0 * w, -2.0 * w][k % 2], y + 0.5, w, h) if k % 4 < 2 else \
                    _floor_point(hcam, x + 0.5, [3.0 * h, -2.0 * h][k % 2], w, h)
            elif cat == "plus_1e300":
                pts[y, x, ch] = 1e300
            elif cat == "minus_1e300":
                pts[y, x] = -1e300
            elif cat == "denormal":
                pts[y, x] = [DENORM64, -3 * DENORM64, 2.0 ** -1030]
            elif cat == "neg_zero":
                pts[y, x, ch] = -0.0
            elif cat == "sub_pixel":
                pts[y, x] = _floor_point(hcam, x + float(rng.uniform(-0.45, 0.45)), y + float(rng.uniform(-0.45, 0.45)), w, h)
            elif cat == "pixels_away":
                pts[y, x] = _floor_point(hcam, x + float(rng.uniform(-6, 6)), y + float(rng.uniform(-6, 6)), w, h)
    return rgb, aov, cur, hist, pts, {c: np.array(v, int) for c, v in planted.items()}


# ---- a deforming mesh: the scene of the real frames ------------------------------------------------------------------------------

def wobble_pose(k):
    """pose k of the animation: a ball of 640 triangles under scale_wobble at phase 0.3 k (tests/scene_update_meshes.py)"""
    import bvh_sweep_meshes as M
    import scene_update_meshes as U
    return np.ascontiguousarray(U.scale_wobble(M.uv_sphere(16, 20, 1.2), phase=0.3 * k))


def mesh_scene(tris, width, height, samples, depth=16):
    """as tests/test_gpu_scene_update.py: a floor-less scene of one light sphere and the mesh, seen from (0, 0, 4)"""
    from rt_amd import abi, scene as S
    objs = [dict(flags=abi.M_DEFAULT, radius=4.0, center=(0, 18, 0), color=(1, 1, 1), emission=(8, 8, 8))]
    return S.custom_scene(objs, width, height, samples, depth, (0, 0, 4), (0, 0, 0),
                          meshes=[dict(flags=abi.M_DEFAULT, color=(0.8, 0.7, 0.6), triangles=np.asarray(tris, dtype=np.float64))])


def pixel_centre_uv(w, h):
    """the grid of step 3 (and of Temporal's query): u = (x + 0.5) / (w - 1), v = (y + 0.5) / (h - 1), row-major [w * h, 2]"""
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([(xs + 0.5) / (w - 1.0), (ys + 0.5) / (h - 1.0)], axis=-1).reshape(-1, 2)
