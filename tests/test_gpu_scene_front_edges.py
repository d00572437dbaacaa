"""The branches of gpu.py's folded scene and ray helpers that the call transcripts (tests/test_scene_front_calls.py) reach and no
other GPU test does: no entries in probe_irradiance and none of the entries in probe_shade, trace_pixels told to trace none of its list, a strided tensor
given to update_spheres / update_vertices, and query_uv writing every field into tensors given.  Bit for bit against the plain call
of the same build, on a room of a dozen spheres and a dozen triangles at 24 x 16."""
import numpy as np
import pytest

from conftest import SEED
from test_gpu_scene_update import assert_same_frame, frame, tris_of
from util import class_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def room():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    gs = G.GpuScene(class_scene(n_packed=4, tris=12, width=24, height=16, samples=2))
    yield G, gs
    gs.close()


def _same(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_no_entries_to_shade(room):
    import torch
    from rt_amd import abi
    G, gs = room
    grid = abi.probe_grid((-1.0, 0.5, -1.0), (2.0, 1.0, 2.0), (2, 1, 2))
    coeff = gs.bake_probe_grid(grid, 2, SEED)
    none = torch.empty((0, 3), dtype=torch.float64, device="cuda")
    assert tuple(G.probe_irradiance(coeff, [], none).shape) == (0, 3)
    # (probe_shade of no points at all is the shim's refusal: an empty tensor goes down as a null pointer.)  Three entries, told to
    # shade none of them, leave what they were given untouched
    pts = torch.tensor([[0.0, 1.0, 0.0], [0.5, 0.75, -0.5], [-0.5, 1.0, 0.5]], dtype=torch.float64, device="cuda")
    nrm = torch.tensor([[0.0, 1.0, 0.0]] * 3, dtype=torch.float64, device="cuda")
    want = G.probe_shade(grid, coeff, pts, nrm)
    kept = dict(irradiance=torch.full((3, 3), 7.0, dtype=torch.float64, device="cuda"), color=torch.full((3, 3), 7.0, device="cuda"))
    G.probe_shade(grid, coeff, pts, nrm, out=kept, m=0)
    got = G.probe_shade(grid, coeff, pts, nrm, out=dict(irradiance=torch.empty_like(want["irradiance"])))
    torch.cuda.synchronize()
    assert float(kept["irradiance"].min()) == 7.0 and float(kept["color"].max()) == 7.0
    assert _same(got["irradiance"], want["irradiance"]) and _same(got["color"], want["color"])


def test_trace_none_of_the_list(room):
    import torch
    G, gs = room
    pixels = torch.tensor([5, 100, 383], dtype=torch.int32, device="cuda")
    none = gs.trace_pixels(pixels, 2, SEED, n=0)
    two = gs.trace_pixels(pixels, 2, SEED, n=2)
    plain = gs.trace_pixels(pixels[:2], 2, SEED)
    torch.cuda.synchronize()
    assert tuple(none["status"].shape) == (0,) and tuple(none["radiance"].shape) == (0, 3) and none["stats"].cpu().tolist() == [0, 0, 0, 0]
    assert all(_same(two[f], plain[f]) for f in ("status", "radiance", "stats"))


def test_a_strided_update_is_copied_not_refused(room):
    import torch
    G, gs = room
    sc = gs.scene
    spheres = gs.spheres().clone()
    spheres[8:, 1] += 0.125
    tris = torch.tensor(tris_of(sc), dtype=torch.float64, device="cuda")
    tris[:, :, 1] += 0.0625
    a, b = G.GpuScene(sc), G.GpuScene(sc)
    try:
        a.update_spheres(spheres)
        a.update_vertices(tris)
        wide_s, wide_t = torch.stack([spheres, spheres + 1.0], dim=-1), torch.stack([tris, tris + 1.0], dim=-1)
        assert not wide_s[..., 0].is_contiguous() and not wide_t[..., 0].is_contiguous()
        b.update_spheres(wide_s[..., 0])
        b.update_vertices(wide_t[..., 0])
        assert _same(b.spheres(), spheres) and b.spheres().is_contiguous()
        assert_same_frame(frame(b), frame(a), "the strided update")
    finally:
        a.close()
        b.close()


def test_query_uv_into_every_field(room):
    import torch
    from rt_amd import abi
    G, gs = room
    uv = torch.tensor([[0.5, 0.5], [0.1, 0.9], [0.95, 0.2], [0.3, 0.3], [0.7, 0.05]], dtype=torch.float64, device="cuda")
    want = gs.query_uv(uv)
    into = {f: torch.full((5, k) if k > 1 else (5,), 7, dtype=G._TORCH[d], device="cuda") for f, (d, k) in abi.HIT_SHAPES.items()}
    got = gs.query_uv(uv, out=into)
    torch.cuda.synchronize()
    assert all(got[f] is into[f] and _same(got[f], want[f]) for f in abi.HIT_FIELDS)
