"""The branches of the previous-points wrappers that the call transcripts (tests/test_image_front_calls.py) reach and no other GPU
test does: no entries in the moved forms with everything else given, where the arrays go down as the "given" address, and three
entries through all four forms, the device ones also in place.  Bit for bit against the same wrapper called the plain way."""
import numpy as np
import pytest

import prev_points_moved_expected as P

pytestmark = pytest.mark.gpu
FIELDS = ("status", "prim", "object", "bary", "point")


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _bits(a):
    import torch
    return (a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint64)


def test_no_entries_with_everything_given(gpu):
    import torch
    hits, prev, cur = P.planted(6, 12)
    none = {f: np.ascontiguousarray(a[:0]) for f, a in hits.items()}
    pos = np.random.default_rng(3).uniform(-4, 4, (12, 3, 3))
    for sp, sc in ((prev, cur), (prev[:0], cur[:0]), (None, None)):
        assert gpu.prev_points_moved_host(none, pos, sp, sc).shape == (0, 3)
        d = {f: _dev(none[f]) for f in FIELDS}
        ds, dc = (None, None) if sp is None else (_dev(sp), _dev(sc))
        assert gpu.prev_points_moved(d, _dev(pos), ds, dc).shape == (0, 3)
        got = gpu.prev_points_moved(d, _dev(pos), ds, dc, out=d["point"])
        torch.cuda.synchronize()
        assert got is d["point"] and got.shape == (0, 3)
    # ... and the card still answers: three entries after the empty calls
    three = {f: np.ascontiguousarray(a[:3]) for f, a in hits.items()}
    assert P.same(gpu.prev_points_moved_host(three, pos, prev, cur), P.prev_points_moved(three, pos, prev, cur))


def test_three_entries_in_place_through_every_form(gpu):
    import torch
    hits, prev, cur = P.planted(6, 12)
    three = {f: np.ascontiguousarray(a[4:7]) for f, a in hits.items()}
    plain = {f: a for f, a in three.items() if f != "object"}
    pos = np.random.default_rng(4).uniform(-4, 4, (12, 3, 3))
    for moved, sp, sc in ((False, None, None), (True, None, None), (True, prev, cur), (True, prev[:0], cur[:0])):
        src = three if moved else plain
        ds, dc = (None, None) if sp is None else (_dev(sp), _dev(sc))
        call = (lambda d, out=None: gpu.prev_points_moved(d, _dev(pos), ds, dc, out=out)) if moved else \
               (lambda d, out=None: gpu.prev_points(d, _dev(pos), out=out))
        want = call({f: _dev(a) for f, a in src.items()})          # the plain way: the output allocated
        d = {f: _dev(a) for f, a in src.items()}
        got = call(d, out=d["point"])
        torch.cuda.synchronize()
        assert got is d["point"] and np.array_equal(_bits(got), _bits(want)), (moved, "in place")
        given = torch.full((3, 3), 7.0, dtype=torch.float64, device="cuda")
        d = {f: _dev(a) for f, a in src.items()}
        assert call(d, out=given) is given
        torch.cuda.synchronize()
        assert np.array_equal(_bits(given), _bits(want)), (moved, "out given")
        host = gpu.prev_points_moved_host(src, pos, sp, sc) if moved else gpu.prev_points_host(src, pos)
        assert np.array_equal(_bits(host), _bits(want)), (moved, "the host form")
