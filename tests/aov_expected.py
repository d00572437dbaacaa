"""The CPU expectation of the first-hit feature buffers (include/rt_hip.h, rt_hip_render_aov_*), built from the compiled
reference: per sample the first two draws of the (seed, pixel, sample) stream (random_doubles), u = (x + r0) / (w - 1) and
v = (y + r1) / (h - 1) as render() forms them (raytracer.c:203-204), get_camera_ray (camera_ray), one intersect() -- the
reference's scan with its mesh block revived (intersect_mesh_scene: the live sphere text, the winner's t, normal and id, and
hit.u / hit.v as the literal block leaves them) -- and checkered_texture (checkered) on M_CHECKERED objects.  Sums in sample
order, one fp64 vec3_add each from 0, times 1.0 / S, rounded to float32 (render(), raytracer.c:199-215).
"""
import numpy as np

BACKGROUND = 10 / 255.0   # raytracer.h: what trace_path returns for a miss, per channel
M_CHECKERED = 16
NO_OBJECT = 0xFFFFFFFF


def _materials(sc):
    """(color, flags) per object id: spheres, then meshes"""
    out = [(sc.objects[i].color.tuple(), int(sc.objects[i].flags)) for i in range(sc.n_objects)]
    out += [(sc.meshes[m].color.tuple(), int(sc.meshes[m].flags)) for m in range(sc.n_meshes)]
    return out


def expected_pixels(ref, sc, seed, samples, pixels, camera=None, extra=None):
    """ref: an oracle_py.RefMeshOracle.  pixels: row-major pixel indices y * w + x.  -> dict of arrays over the pixels, as the
    device buffers hold them: albedo / normal float32 [n,3], depth float32 [n], object / hits uint32 [n].
    extra: a dict that receives what the buffers do not show -- t_min float64 [n] (the depth before its rounding to float32)
    and checker uint32 [n,2]: how many of the pixel's samples hit an M_CHECKERED object and took its 0.3x / its 0.7x albedo"""
    cam = camera if camera is not None else sc.camera
    w, h = sc.width, sc.height
    mats = _materials(sc)
    pixels = np.asarray(pixels, dtype=np.int64).ravel()
    n = len(pixels)
    out = dict(albedo=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32), depth=np.zeros(n, np.float32),
               object=np.zeros(n, np.uint32), hits=np.zeros(n, np.uint32))
    inv = 1.0 / float(samples)
    t64, checker = np.full(n, np.inf), np.zeros((n, 2), np.uint32)
    for k, p in enumerate(pixels):
        x, y = int(p % w), int(p // w)
        alb, nrm = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        t_min, obj, hits = float("inf"), NO_OBJECT, 0
        for s in range(samples):
            r = ref.random_doubles(seed, int(p), s, 2)
            u = (float(x) + r[0]) / (float(w) - 1.0)
            v = (float(y) + r[1]) / (float(h) - 1.0)
            hit = ref.intersect_mesh_scene(ref.camera_ray(cam, u, v), sc)
            if hit["hit"]:
                color, flags = mats[hit["id"]]
                a = ref.checkered(color, hit["u"], hit["v"], 100000.0) if flags & M_CHECKERED else color
                if flags & M_CHECKERED:
                    c = int(np.argmax(color))
                    checker[k, int(float(a[c]) > 0.5 * float(color[c]))] += 1
                nn = hit["normal"]
                hits += 1
                if hit["min_t"] < t_min:
                    t_min, obj = hit["min_t"], hit["id"]
            else:
                a, nn = (BACKGROUND, BACKGROUND, BACKGROUND), (0.0, 0.0, 0.0)
            alb = [alb[c] + float(a[c]) for c in range(3)]
            nrm = [nrm[c] + float(nn[c]) for c in range(3)]
        out["albedo"][k] = [alb[c] * inv for c in range(3)]
        out["normal"][k] = [nrm[c] * inv for c in range(3)]
        out["depth"][k] = t_min
        out["object"][k] = obj
        out["hits"][k] = hits
        t64[k] = t_min
    if extra is not None:
        extra["t_min"], extra["checker"] = t64, checker
    return out


def expected_image(ref, sc, seed, samples, camera=None, extra=None):
    """expected_pixels over the whole image, shaped as GpuScene.aov_image returns it (extra: flat over the pixels)"""
    w, h = sc.width, sc.height
    e = expected_pixels(ref, sc, seed, samples, np.arange(w * h), camera, extra)
    return {f: (a.reshape(h, w, 3) if a.ndim == 2 else a.reshape(h, w)) for f, a in e.items()}


def mismatch(got, exp):
    """'' when every buffer is equal bit for bit, else a description of the first differences"""
    msgs = []
    for f in ("albedo", "normal", "depth", "object", "hits"):
        g, e = np.ascontiguousarray(got[f]), np.ascontiguousarray(exp[f])
        if g.shape != e.shape:
            msgs.append(f"{f}: shape {g.shape} != {e.shape}")
            continue
        gb, eb = g.view(np.uint32), e.view(np.uint32)
        bad = np.argwhere(gb != eb)
        if len(bad):
            i = tuple(bad[0])
            msgs.append(f"{f}: {len(bad)} words differ, first at {i}: got {g[i]!r} expected {e[i]!r}")
    return "; ".join(msgs)
