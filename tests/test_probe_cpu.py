"""The light probes' restatement (tests/probe_expected.py) on the CPU: the vectorised form equals the scalar form bit for bit on the
sets the GPU tests use; the all-reject path, which chance does not reach, through a patched draw source; what the contract means --
unit directions, an orthonormal basis under the sampler, a hemisphere that integrates the cosine to pi --; and every refusal of the
shim that needs no device."""
import ctypes as C

import numpy as np
import pytest

import probe_expected as P


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def test_vectorised_equals_scalar_on_the_gpu_sets():
    checked = 0
    for n, s in P.SETS:
        for dist in P.DISTANCES:
            pos, nrm = P.positions(n, dist), P.normals(n)
            for normals, bias in ((None, 0.0), (nrm, 0.0), (nrm, 2.0 ** -10)):
                vec, rejected = P.probe_rays(pos, normals, s, P.SEED, bias=bias, info=True)
                for k in range(n * s):
                    ray, rej = P.probe_ray_scalar(pos, normals, s, P.SEED, k, bias)
                    assert (_bits(ray) == _bits(vec[k])).all() and rej == rejected[k], (n, s, dist, bias, k)
                    checked += 1
                for first, m in P.sub_ranges(n, s):
                    part = P.probe_rays(pos, normals, s, P.SEED, first, m, bias)
                    assert part.shape == (m, 6) and (_bits(part) == _bits(vec[first:first + m])).all()
    print(f"{checked} rays: the vectorised form equals the scalar form bit for bit")


def test_fold_resolve_and_irradiance_vectorised_equal_scalar():
    rng = np.random.default_rng(7)
    n, s = 5, 13
    pos, nrm = P.positions(n, 1.0), P.normals(n)
    rad = rng.uniform(0.0, 4.0, (n * s, 3))
    for normals in (None, nrm):
        rays = P.probe_rays(pos, normals, s, P.SEED)
        total = P.fold(rays, rad, s, normals)
        for i in range(n):
            for j in range(total.shape[1]):
                for c in range(3):
                    assert _bits(P.fold_scalar(rays, rad, s, i, j, c, normals)) == _bits(total[i, j, c]), (i, j, c)
    coeff, _ = P.resolve(P.fold(P.probe_rays(pos, None, s, P.SEED), rad, s), s, P.SPHERE)
    index = np.array([0, 4, 2, 5, 1])
    E = P.irradiance(coeff, index, nrm)
    for e in range(5):
        for c in range(3):
            want = P.irradiance_scalar(coeff, int(index[e]), [float(v) for v in nrm[e]], c)
            assert (np.isnan(want) and np.isnan(E[e, c])) or _bits(want) == _bits(E[e, c]), (e, c)
    assert np.isnan(E[3]).all() and np.isfinite(E[[0, 1, 2, 4]]).all()


def test_the_sets_reach_several_counts_of_rejected_rounds():
    """a round rejects with probability 1 - pi / 6 = 0.476: 0, 1, 2 and >= 3 rejected rounds must all occur in the GPU tests' sets"""
    seen = np.zeros(P.ROUNDS + 1, dtype=np.int64)
    for n, s in P.SETS:
        _, rejected = P.probe_rays(P.positions(n, 1.0), None, s, P.SEED, info=True)
        seen += np.bincount(rejected, minlength=P.ROUNDS + 1)
    print("rejected rounds -> rays:", {k: int(v) for k, v in enumerate(seen) if v})
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 0 and seen[3:P.ROUNDS].sum() > 0
    assert seen[P.ROUNDS] == 0, "all 32 rounds rejecting has probability 0.476^32 = 5e-11: these sets do not reach it"


def test_all_rounds_rejecting_gives_plus_z():
    pos, nrm = P.positions(3, 1.0), np.array([[0.0, 0.0, -1.0]] * 3)
    draws = []

    def corner():
        draws.append(1)
        return 0.999   # x = y = z = 0.998: q > 1 in every round
    ray, rejected = P.probe_ray_scalar(pos, None, 4, P.SEED, 5, draw=corner)
    assert len(draws) == 3 * P.ROUNDS and rejected == P.ROUNDS
    assert ray[3:] == (0.0, 0.0, 1.0) and ray[:3] == tuple(pos[1])
    ray, _ = P.probe_ray_scalar(pos, nrm, 4, P.SEED, 5, bias=0.5, draw=lambda: 0.999)
    assert ray[3:] == (-0.0, -0.0, -1.0) and ray[:3] == tuple(pos[1] + nrm[1] * 0.5), "the fallback is flipped like any direction"
    tiny = iter([0.5, 0.5, 0.5 + 2.0 ** -12] * 1 + [0.75, 0.5, 0.5] * 40)   # q = 2^-22 < 2^-20: rejected; then (0.5, 0, 0)
    ray, rejected = P.probe_ray_scalar(pos, None, 4, P.SEED, 0, draw=lambda: next(tiny))
    assert rejected == 1 and ray[3:] == (1.0, 0.0, 0.0)


def test_directions_are_unit():
    for n, s in P.SETS + ((1, 4096),):
        rays = P.probe_rays(P.positions(n, 1.0), P.normals(n), s, P.SEED, bias=2.0 ** -10)
        d = rays[:, 3:]
        q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert (np.abs(q - 1.0) <= 2.0 ** -50).all(), float(np.abs(q - 1.0).max())


def test_gram_matrix_is_the_identity():
    """One probe, S = 4096, seed 20261020: G_jk = (4 pi / S) sum_s w_j w_k is within 6 standard errors of the identity, the standard
    error of each entry computed from its own 4096 terms (plus 2^-50, the rounding of the literals: G_00's terms are all Y0*Y0 and
    its standard error is 0).  The seed was chosen here, on the CPU; the worst ratio |G_jk - I_jk| / SE over the 44 entries with a
    spread is 2.33 (G_37, recorded from this run)."""
    s = 4096
    w = P.sh_bases(P.probe_rays(np.zeros((1, 3)), None, s, P.SEED)[:, 3:])
    terms = 4.0 * np.pi * w[:, :, None] * w[:, None, :]
    G = terms.mean(axis=0)
    se = terms.std(axis=0, ddof=1) / np.sqrt(s)
    err = np.abs(G - np.eye(9))
    ratio = np.where(se > 0, err / np.where(se > 0, se, 1.0), 0.0)
    j, k = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"worst ratio {ratio.max():.2f} at G[{j}][{k}]; |G_00 - 1| = {err[0, 0]:.3g}")
    assert (err <= 6.0 * se + 2.0 ** -50).all(), (ratio.max(), j, k)


def test_hemisphere_flips_and_integrates_the_cosine():
    """every flipped direction has c >= 0, and 2 pi mean(c) is within 6 standard errors of pi (S = 4096, unit normal)"""
    s = 4096
    n = np.array([[2.0, -1.0, 2.0]]) / 3.0
    rays = P.probe_rays(np.zeros((1, 3)), n, s, P.SEED, bias=0.25)
    d = rays[:, 3:]
    c = (d[:, 0] * n[0, 0] + d[:, 1] * n[0, 1]) + d[:, 2] * n[0, 2]
    assert (c >= 0).all()
    assert (_bits(rays[:, :3]) == _bits(np.zeros((1, 3)) + n * 0.25)).all()
    free = P.probe_rays(np.zeros((1, 3)), None, s, P.SEED)[:, 3:]
    flipped = (_bits(free) != _bits(d)).any(axis=1)
    assert 0.4 * s < flipped.sum() < 0.6 * s and (_bits(free[flipped] * -1.0) == _bits(d[flipped])).all()
    terms = 2.0 * np.pi * P.cos_basis(d, np.repeat(n, s, axis=0))[:, 0]
    se = terms.std(ddof=1) / np.sqrt(s)
    print(f"2 pi mean(c) = {terms.mean():.5f}, standard error {se:.5f}: {abs(terms.mean() - np.pi) / se:.2f} of them from pi")
    assert abs(terms.mean() - np.pi) <= 6.0 * se


# ---- refusals: arguments are checked before a device is looked for ----------------------------------------------------------------------------
def test_refusals_need_no_device():
    from rt_amd import abi, scene as S
    shim = abi.load_shim()
    EINVAL, ENODEV = -2, -1
    sc = S.build_scene(1, 16, 16, 1)
    n = 4
    pos, nrm = np.ascontiguousarray(P.positions(n, 1.0)), np.ascontiguousarray(P.normals(n))
    coeff = np.full((n, 9, 3), 7.0)
    fake = 0x1000   # an aligned address nothing dereferences: every call below is refused before a launch

    def host(mode=abi.PROBE_SPHERE, samples=8, normals=False, n_probes=n, positions=True, out=True, device=99, **fields):
        p = abi.probe_params(mode, samples, P.SEED, 4)
        for k, v in fields.items():
            setattr(p, k, v)
        return shim.rt_hip_bake_probes_host(sc.objects, sc.n_objects, None, 0, pos.ctypes.data if positions else None,
                                            nrm.ctypes.data if normals else None, n_probes, C.byref(p), device,
                                            coeff.ctypes.data if out else None, None, None, None)

    def device_form(slice_rays=64, ws=fake, scene=fake, d_sum=None, d_coeff=fake, positions=fake, n_probes=n, **fields):
        p = abi.probe_params(abi.PROBE_SPHERE, 8, P.SEED, 4)
        for k, v in fields.items():
            setattr(p, k, v)
        return shim.rt_hip_bake_probes(C.c_void_p(scene), C.c_void_p(positions), None, n_probes, C.byref(p), slice_rays, C.c_void_p(ws),
                                       C.c_void_p(d_sum), C.c_void_p(d_coeff), None, None, None, None)

    cases = {
        "unknown mode": dict(mode=2), "flags": dict(flags=1), "reserved": dict(reserved=1), "samples 0": dict(samples=0),
        "probes x samples > 2^32": dict(n_probes=2 ** 16 + 1, samples=2 ** 16), "bias < 0": dict(bias=-1e-9), "bias NaN": dict(bias=float("nan")),
        "bias inf": dict(bias=float("inf")), "origin_radius < 0": dict(origin_radius=-1.0), "origin_radius NaN": dict(origin_radius=float("nan")),
        "origin_radius inf": dict(origin_radius=float("inf")), "hemisphere without normals": dict(mode=abi.PROBE_HEMISPHERE),
        "max_depth < 0": dict(max_depth=-1), "max_depth > 1000000": dict(max_depth=1000001), "no positions": dict(positions=False),
        "no coeff": dict(out=False),
    }
    for what, kw in cases.items():
        assert host(**kw) == EINVAL, (what, shim.rt_hip_last_error())
    assert host() == ENODEV, "a valid call looks for logical device 99, and there is none"
    assert host(mode=abi.PROBE_HEMISPHERE, normals=True, bias=0.5) == ENODEV
    assert host(n_probes=0, positions=False, out=False) == 0, "no probe: nothing to do, on any device or none"
    assert (coeff == 7.0).all()
    device_cases = {
        "slice_rays 0": dict(slice_rays=0), "workspace not 16-byte aligned": dict(ws=fake + 8), "sum not 8-byte aligned": dict(d_sum=fake + 4),
        "no scene": dict(scene=None), "no workspace": dict(ws=None), "no coeff": dict(d_coeff=None), "no positions": dict(positions=None),
        "samples 0": dict(samples=0), "flags": dict(flags=2), "bias < 0": dict(bias=-1.0),
    }
    for what, kw in device_cases.items():
        assert device_form(**kw) == EINVAL, (what, shim.rt_hip_last_error())
    assert device_form(slice_rays=0) == EINVAL and b"slice_rays" in shim.rt_hip_last_error()
    assert device_form(ws=fake + 8) == EINVAL and b"16-byte" in shim.rt_hip_last_error()
    assert device_form(n_probes=0, scene=None, ws=None, d_coeff=None, positions=None) == 0
    # the generator, the resolve and the evaluation
    p = abi.probe_params(abi.PROBE_SPHERE, 8, P.SEED)
    gen = lambda k_first=0, m=8, rays=fake, positions=fake, params=p, n_probes=n: shim.rt_hip_probe_rays(
        C.c_void_p(positions), None, n_probes, C.byref(params) if params is not None else None, k_first, m, C.c_void_p(rays), None)
    assert gen(rays=fake + 8) == EINVAL and gen(rays=None) == EINVAL and gen(positions=None) == EINVAL and gen(params=None) == EINVAL
    assert gen(k_first=n * 8, m=1) == EINVAL and gen(k_first=1, m=n * 8) == EINVAL
    assert gen(params=abi.probe_params(abi.PROBE_HEMISPHERE, 8, P.SEED)) == EINVAL and gen(params=abi.probe_params(3, 8, P.SEED)) == EINVAL
    assert gen(m=0, rays=None) == 0 and gen(k_first=n * 8, m=0) == 0
    # good arguments: the device that holds d_rays is looked for -- none here; where there is one, `fake` is not its memory
    assert gen() == (ENODEV if shim.rt_hip_device_count() == 0 else EINVAL)
    assert shim.rt_hip_probe_resolve(C.c_void_p(fake), n, 2, 8, C.c_void_p(fake), None, None) == EINVAL
    assert shim.rt_hip_probe_resolve(C.c_void_p(fake), n, 0, 0, C.c_void_p(fake), None, None) == EINVAL
    assert shim.rt_hip_probe_resolve(None, n, 0, 8, C.c_void_p(fake), None, None) == EINVAL
    assert shim.rt_hip_probe_resolve(C.c_void_p(fake), n, 0, 8, None, None, None) == EINVAL
    assert shim.rt_hip_probe_irradiance(C.c_void_p(fake), n, None, C.c_void_p(fake), 3, C.c_void_p(fake), None) == EINVAL
    assert shim.rt_hip_probe_irradiance(C.c_void_p(fake), n, C.c_void_p(fake), C.c_void_p(fake), 3, None, None) == EINVAL
    assert shim.rt_hip_probe_irradiance(None, n, None, None, 0, None, None) == 0
    assert shim.rt_hip_probe_workspace_bytes(n, 2, 64) == 0 and shim.rt_hip_probe_workspace_bytes(n, 0, 0) == 0
    assert shim.rt_hip_probe_workspace_bytes(n, 0, 64) >= 76 * 64 + 24 * 9 * n
    assert shim.rt_hip_probe_workspace_bytes(n, 1, 64) >= 76 * 64 + 24 * n
    q = abi.RtHipProbeParams()
    shim.rt_hip_probe_defaults(C.byref(q))
    assert (q.mode, q.flags, q.samples, q.max_depth, q.seed, q.bias, q.origin_radius, q.reserved) == (0, 0, 64, 5, 0, 0.0, 0.0, 0)
    assert C.sizeof(abi.RtHipProbeParams) == 48
    sc.free()
