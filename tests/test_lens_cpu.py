"""The lens ray's restatement (tests/lens_expected.py) on the CPU: the vectorised form equals the scalar form bit for bit on the sets
the GPU tests use; what those sets reach (pixels with 0, 1, 2 and at least 3 rejected rounds; the all-reject path, which chance does
not reach, through a patched draw source); and the geometry of the contract (origins on the lens disk, every ray through its own
focus point, the disk sampler's second moment)."""
import numpy as np
import pytest

import lens_expected as L
import util


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def cameras():
    """the class scene's own camera and two others, far and off-axis (tests/util.py, view_variant)"""
    base = util.class_scene(n_packed=4, width=17, height=9)
    out = {"own": L.camera_tuple(base.camera)}
    for name in ("far", "sheared"):
        sc = util.view_variant(base, name)
        out[name] = L.camera_tuple(sc.camera)
        sc.free()
    base.free()
    return out


def test_vectorised_equals_scalar_on_the_gpu_sets(cameras):
    checked = 0
    for (w, h) in L.FRAMES:
        for sample in L.SAMPLES:
            for name, cam in cameras.items():
                for R in L.APERTURES:
                    for f in L.FOCUSES:
                        if (R, f) not in ((0.5, 1.0), (0.0, 1e-3), (2.0 ** -10, 1e3)) and (w, h, name) != (17, 9, "own"):
                            continue   # the full cross product on one frame and camera, three corners of it on the others
                        vec, info = L.lens_rays(cam, w, h, R, f, L.SEED, sample, info=True)
                        for p in range(w * h):
                            ray, one = L.lens_ray_scalar(cam, w, h, R, f, L.SEED, sample, p)
                            assert (_bits(ray) == _bits(vec[p])).all(), (w, h, sample, name, R, f, p)
                            assert one["rejected"] == info["rejected"][p] and one["a"] == info["a"][p]
                            checked += 1
    print(f"{checked} rays: the vectorised form equals the scalar form bit for bit")
    for first, n in L.sub_ranges(65 * 3):
        part = L.lens_rays(cameras["own"], 65, 3, 0.5, 1.0, L.SEED, 1, first, n)
        whole = L.lens_rays(cameras["own"], 65, 3, 0.5, 1.0, L.SEED, 1)
        assert (_bits(part) == _bits(whole[first:first + n])).all()


def test_the_sets_reach_every_count_of_rejected_rounds(cameras):
    """a round rejects with probability 1 - pi / 4 = 0.215: 0, 1, 2 and >= 3 rejected rounds must all occur in the GPU tests' frames"""
    seen = np.zeros(L.ROUNDS + 1, dtype=np.int64)
    for (w, h) in L.FRAMES:
        for sample in L.SAMPLES:
            _, info = L.lens_rays(cameras["own"], w, h, 0.5, 1.0, L.SEED, sample, info=True)
            seen += np.bincount(info["rejected"], minlength=L.ROUNDS + 1)
    print("rejected rounds -> rays:", {k: int(v) for k, v in enumerate(seen) if v})
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 0 and seen[3:L.ROUNDS].sum() > 0
    assert seen[L.ROUNDS] == 0, "all 32 rounds rejecting has probability 0.215^32 = 4e-22: chance does not reach it"


def test_all_rounds_rejecting_gives_the_centre_of_the_lens(cameras):
    cam = cameras["own"]
    draws = []

    def corner():
        draws.append(1)
        return 0.999   # a = b = 0.998: a*a + b*b > 1 in every round
    ray, info = L.lens_ray_scalar(cam, 17, 9, 0.5, 3.0, L.SEED, 0, 40, lens_draw=corner)
    assert len(draws) == 2 * L.ROUNDS and info["rejected"] == L.ROUNDS and info["a"] == 0.0 and info["b"] == 0.0
    assert ray[:3] == cam[0], "the centre of the lens is the camera position"
    free, _ = L.lens_ray_scalar(cam, 17, 9, 0.0, 3.0, L.SEED, 0, 40)
    assert ray == free, "and the ray is the aperture-0 ray of that pixel and sample"


def test_geometry(cameras):
    """Origins.  L is position + (ax*(a*R) + ay*(b*R)) to the bit, so the bound is checked on the offset itself, where the rounding of
    the sum with a far position plays no part.  With a*a + b*b < 1 and unit axes |a ax + b ay|^2 = a^2 + b^2 + 2 a b (ax . ay)
    <= (a^2 + b^2)(1 + |ax . ay|): within R (1 + 2^-50) of the position for a camera whose horizontal and vertical are orthogonal (the
    scene's own, the far one), within R sqrt(1 + |ax . ay|) (1 + 2^-50) for a sheared one (rt_hip.h says so)."""
    for name, cam in cameras.items():
        pos = np.array(cam[0])
        ax, ay = np.array(L._normalize3(cam[1])), np.array(L._normalize3(cam[2]))
        shear = abs(float(ax @ ay))
        assert (shear <= 2.0 ** -50) == (name != "sheared"), (name, shear)
        normal = np.cross(ax, ay)
        normal /= np.linalg.norm(normal)
        for R in L.APERTURES:
            for f in L.FOCUSES:
                rays, info = L.lens_rays(cam, 17, 9, R, f, L.SEED, 1, info=True)
                off = ax[None, :] * (info["a"] * R)[:, None] + ay[None, :] * (info["b"] * R)[:, None]
                assert (_bits(rays[:, :3]) == _bits(pos[None, :] + off)).all(), (name, R, f)
                reach = R * (1.0 + 2.0 ** -50) * (np.sqrt(1.0 + shear) if name == "sheared" else 1.0)
                assert (np.linalg.norm(off, axis=1) <= reach).all(), (name, R, f)
                assert (np.abs(off @ normal) <= 2.0 ** -50 * R).all(), (name, R, f)
                # every ray passes its own focus point: the distance of F from the line L + t q, relative to |F - L|
                e = info["F"] - rays[:, :3]
                q = rays[:, 3:]
                miss = np.linalg.norm(np.cross(e, q), axis=1)
                assert (miss <= 2.0 ** -45 * np.linalg.norm(e, axis=1)).all(), (name, R, f, float((miss / np.linalg.norm(e, axis=1)).max()))
                assert (np.abs((q * q).sum(axis=1) - 1.0) <= 2.0 ** -50).all()


def test_optics_scene_shows_depth_of_field(pt):
    """The scene of the GPU suite's optics test, chosen here: an emitter of radius 0.15 on the focal plane (1.5 ahead) and one of
    radius 0.3 at 3.0, 33 x 17 pixels (0.10 wide on the focal plane), 64 samples.  Lit pixels from the restated rays: aperture 0: 12
    and 12 (the same pinhole footprint); aperture 0.25: 12 and 24 -- the far sphere's edge blurs by R (3.0 - 1.5) / 1.5 = 0.25, more
    than a pixel (0.20 at that depth).  The oracle's intersect_sphere agrees with the sphere test used, ray for ray, on one pass."""
    got = {}
    for k in (1, 2):
        sc = L.optics_scene(k)
        for R in (0.0, L.OPTICS["aperture"]):
            got[(R, k)] = int(L.optics_lit(sc, R).sum())
        rays, hit = L.optics_hits(sc, L.OPTICS["aperture"], 0)
        c, rad = sc.objects[1].center.tuple(), float(sc.objects[1].radius)
        assert [bool(pt.intersect_sphere(ray, c, rad)[0]) for ray in rays] == hit.tolist()
        sc.free()
    print("lit pixels (aperture, k):", got)
    assert got == L.OPTICS_LIT
    assert got[(0.25, 2)] >= 2 * got[(0.25, 1)] and got[(0.0, 1)] == got[(0.0, 2)]


def test_disk_sampler_second_moment(cameras):
    """uniform on the unit disk: E[a*a + b*b] = 1/2, standard deviation sqrt(1/12) = 0.289; over 4096 samples the mean's is 0.0045,
    so 0.5 +- 0.05 is eleven of them.  Seed 20261020, pixel 0 of a 2 x 2 frame, samples 0 .. 4095: 0.5022"""
    cam = cameras["own"]
    r2 = []
    for s in range(4096):
        _, info = L.lens_rays(cam, 2, 2, 1.0, 1.0, L.SEED, s, 0, 1, info=True)
        r2.append(float(info["a"][0] * info["a"][0] + info["b"][0] * info["b"][0]))
    mean = float(np.mean(r2))
    print(f"mean of a*a + b*b over 4096 samples: {mean:.4f}")
    assert abs(mean - 0.5) <= 0.05
