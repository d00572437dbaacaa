"""The other half of rt_amd/gpu.py pinned the way tests/test_image_front_calls.py pins the image-space wrappers, with that module's
Recorder, Names, _normalise, _patch and scene_stub: GpuScene from its constructor to render_image, the rest of Accumulation, Preview,
and the host forms and generators from render_image_host to bake_probes_host.  No device and no built shim.  On top of the image
recorder, SceneRecorder answers what these wrappers read back (a device count, kernel names, handles, what a case plants behind an
address), describes an out-parameter as "out:<ctype>" and a ctypes array as "array:<ctype>", and records torch.cuda.synchronize and a
stream's synchronize() as calls of their own.  Recorded from the tree before this half was folded
(tests/golden/scene_front_calls.json; `python tests/test_scene_front_calls.py --record` writes the file) and must not move."""
import ctypes as C
import dataclasses
import functools
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracer.c_amd"))

from test_image_front_calls import (CPU, F32, F64, I32, I64, SCENE, STREAM, U8, H, W, Names, Recorder, _BYREF, _is_host,  # noqa: E402
                                    _normalise, _patch, scene_stub, strided, z)

from rt_amd import abi, gpu  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_front_calls.json")
ACCUM = 0xACC00000


# ---- the recorder ------------------------------------------------------------------------------------------------------------------------------
def _address(a):
    return a.value if isinstance(a, C.c_void_p) else a


EMPTY = 0xE3B0E3B0   # the "first word" of an array of no entries: there is none to read


def _empties():
    """the addresses of the empty arrays that the wrappers on the stack hold (in a local, or in a local dict)"""
    out, frame = set(), sys._getframe(2)
    while frame is not None and frame.f_code.co_filename == gpu.__file__:
        for v in list(frame.f_locals.values()):
            out.update(a.ctypes.data for a in (v.values() if isinstance(v, dict) else [v]) if isinstance(a, np.ndarray) and a.size == 0)
        frame = frame.f_back
    return out


class SceneRecorder(Recorder):
    """the image recorder plus: answers[symbol] (a value, or a function of the arguments) is what a symbol returns, effects[symbol]
    (a function of the arguments) plants what the wrapper reads back; a created handle is SCENE or ACCUM + 256 k"""

    def __init__(self, names=None):
        super().__init__(names)
        self.answers, self.effects, self.handles = {"rt_hip_device_count": 1}, {}, 0

    def __getattr__(self, symbol):
        def call(*args):
            types_ = abi.SHIM_SYMBOLS[symbol][1]
            shown, special, words = list(args), {}, {}
            unnamed = lambda v: self.names is not None and v not in (None, 0, 1, STREAM) and v not in self.names
            empties = _empties() if _is_host(symbol) else ()
            word = lambda v: EMPTY if v in empties else C.c_uint32.from_address(v).value
            for k, a in enumerate(args):
                obj = a._obj if isinstance(a, _BYREF) else a
                if isinstance(obj, C.c_void_p) and isinstance(a, _BYREF):   # a handle to create
                    obj.value = SCENE if "scene" in symbol else ACCUM + 256 * self.handles
                    self.handles += "scene" not in symbol
                    if self.names is not None:
                        self.names.add(("scene" if "scene" in symbol else "accum") + "#%d" % self.handles, C.c_void_p(obj.value))
                if (isinstance(a, _BYREF) and isinstance(obj, (C._SimpleCData, C.Array))) or isinstance(a, C.Array):
                    special[k] = ("out:" if isinstance(a, _BYREF) else "array:") + type(obj).__name__
                    shown[k] = None
                elif isinstance(obj, C.Structure) and _is_host(symbol):
                    for f, t in obj._fields_:
                        v = getattr(obj, f)
                        if t is C.c_void_p and unnamed(v):
                            words[v] = word(v)
                elif types_[k] is C.c_void_p and _is_host(symbol) and unnamed(_address(a)):
                    words[_address(a)] = word(_address(a))
            if self.names is not None:
                got = _normalise(self.names, symbol, shown, words)
                for k, what in special.items():
                    got[1][k] = what
                self.calls.append(got)
            if symbol in self.effects:
                self.effects[symbol](*args)
            if symbol in self.answers:
                r = self.answers[symbol]
                return r(*args) if callable(r) else r
            if symbol.endswith("kernel_name") or symbol in ("rt_hip_last_launch_kernel", "rt_hip_accum_kernel"):
                return ("kernel of " + symbol).encode()
            if symbol == "rt_hip_last_error":
                return b"the recorder's error"
            return 64 if symbol.endswith("_workspace_bytes") else 0
        return call


def _patch_scene(mp, rec):
    _patch(mp, rec)

    def note(what, *a):
        if rec.names is not None:
            rec.calls.append([what, list(a)])
    mp.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(
        cuda_stream=STREAM, synchronize=lambda: note("stream.synchronize", str(device))))
    mp.setattr(torch.cuda, "synchronize", lambda device=None: note("torch.cuda.synchronize", str(device)))
    kept = []   # what a wrapper allocates lives to the end of the case: no address is given out twice, so none gets another buffer's name

    def keeping(make):
        def made(*a, **kw):
            kept.append(make(*a, **kw))
            return kept[-1]
        return made
    for f in ("empty", "zeros", "empty_like"):
        mp.setattr(torch, f, keeping(getattr(torch, f)))
    rec.kept = kept


def _transcript(mp, fn):
    names = Names()
    rec = SceneRecorder(names)
    _patch_scene(mp, rec)
    ret = fn(rec, names)
    calls = names.settle(rec.calls, ret)
    rec.names = None   # (what dies from here on is not part of the case)
    return json.loads(json.dumps(dict(calls=calls, returns=names.describe(ret))))


def _refusal(mp, fn):
    rec = SceneRecorder()
    _patch_scene(mp, rec)
    with pytest.raises((ValueError, gpu.ShimError)) as e:
        fn(rec, Names())
    return "%s: %s" % (type(e.value).__name__, e.value)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class StubScene:
    """what gpu.py reads of a scene.Scene (a dataclass: Preview makes its low scene with dataclasses.replace)"""
    width: int = W
    height: int = H
    samples: int = 4
    max_depth: int = 5
    camera: object = None
    objects: object = None
    n_objects: int = 2
    n_meshes: int = 1
    n_triangles: int = 3

    def hip_meshes(self):
        return "meshes"


def host_scene(names, **kw):
    objs = (abi.Object * 2)()
    for k in range(2):
        objs[k].radius, objs[k].center.x, objs[k].center.y, objs[k].center.z = 0.5 + k, 1.0 + k, 2.0 + k, 3.0 + k
    return StubScene(camera=names.add("scene.camera", abi.Camera()), objects=objs, **kw)


def stub(rec, names, **kw):
    """scene_stub's GpuScene with the whole StubScene under it; it lives to the end of the case"""
    gs = scene_stub(rec, names)
    gs.scene = StubScene(camera=gs.scene.camera, objects=host_scene(Names()).objects, **kw)
    names.keep.append(gs)
    return gs


def record(p):
    """a ctypes record the wrapper returned, field by field"""
    return {f: (list(v) if isinstance(v, C.Array) else v) for f, v in ((f, getattr(p, f)) for f, _ in p._fields_)}


def off16(*shape, dtype=F64):
    """zeros of this shape in a view that starts 8 bytes off a 16-byte boundary"""
    n = int(np.prod(shape))
    base = torch.zeros(n + 3, dtype=dtype)
    t = base[(1 if base.data_ptr() % 16 == 0 else 2):][:n].reshape(shape)
    assert t.data_ptr() % 16 == 8
    return t


class OnDevice(torch.Tensor):
    """a host tensor that says it lies on a device: the branch of the updates that waits for torch's current stream"""
    is_cuda = property(lambda self: True)


def grid(count=(2, 1, 2)):
    return abi.probe_grid((-1.0, 0.5, -3.0), (2.0, 1.0, 1.5), count)


def plant(address_of, ctype, value):
    """an effect: writes value behind the address address_of(args) finds"""
    def effect(*args):
        ctype.from_address(address_of(*args)).value = value
    return effect


T, R = {}, {}


def case(name, *kinds):
    def register(fn):
        for k in kinds or (None,):
            T[name if k is None else f"{name}-{k}"] = (lambda rec, names, k=k: fn(rec, names, k)) if kinds else fn
        return fn
    return register


def refusal(name, *kinds):
    def register(fn):
        for k in kinds:
            R[f"{name}-{k}"] = (lambda rec, names, k=k: fn(rec, names, k))
        return fn
    return register


# ---- plain scene calls -------------------------------------------------------------------------------------------------------------------------------
@case("scene_init", "host", "device")
def _(rec, names, kind):
    gs = gpu.GpuScene(names.add("scene.description", host_scene(names)), device=2, bvh=kind)
    names.keep.append(gs)
    return dict(handle=names[gs.handle.value], device=gs.device, meshes=gs._meshes, accums=gs._accums)


@refusal("scene_init", "bad_bvh", "no_device", "first_bvh_then_device")
def _(rec, names, kind):
    if kind != "bad_bvh":
        rec.answers["rt_hip_device_count"] = 0
    gpu.GpuScene(host_scene(names), bvh="host" if kind == "no_device" else "gpu")


@case("scene_close", "open_accumulation", "closed_accumulation", "twice")
def _(rec, names, kind):
    gs = gpu.GpuScene(host_scene(names))
    names.keep.append(gs)
    a, b = gs.accumulate(7, 4), gs.accumulate(8, 4)
    names.keep.extend([a, b])
    if kind == "closed_accumulation":
        a.close()
    held = [h.value and names[h.value] for h in gs._accums]
    gs.close()
    if kind == "twice":
        gs.close()
    return dict(held=held, handle=gs.handle, accumulations=[a.handle.value, b.handle.value], accums=gs._accums)


@case("params", "defaults", "given")
def _(rec, names, kind):
    gs = stub(rec, names)
    return record(gs.params(7, 1, 2, 3) if kind == "defaults" else gs.params(7, 1, 2, 3, samples=9, max_depth=0, integrator="whitted"))


@case("suggest_chunks", "defaults", "given", "depth_0")
def _(rec, names, kind):
    gs = stub(rec, names)
    rec.answers["rt_hip_suggest_chunks_depth"] = 3
    return gs.suggest_chunks(6, **dict(defaults={}, given=dict(samples=9, max_depth=2), depth_0=dict(samples=0, max_depth=0))[kind])


@case("accumulate", "defaults", "given", "after_a_close")
def _(rec, names, kind):
    gs = stub(rec, names)
    kw = dict(max_depth=0, integrator="whitted", first=1, stride=2, count=1, camera=names.add("camera", abi.Camera())) if kind == "given" else {}
    if kind == "after_a_close":
        gs.accumulate(1, 2).close()
    acc = gs.accumulate(7, 4, **kw)
    names.keep.append(acc)
    return dict(handle=names[acc.handle.value], count=acc.count, seed=acc.seed, first=acc.first, stride=acc.stride,
                camera=None if acc.camera is None else names[C.addressof(acc.camera)], scene=acc.gs is gs,
                accums=[names[h.value] for h in gs._accums])


@case("names_and_status")
def _(rec, names):
    gs = stub(rec, names)
    rec.effects["rt_hip_launch_status"] = lambda device, flags: setattr(flags._obj, "value", 0)
    return dict(kernel=gs.kernel_name(), whitted=gs.kernel_name("whitted"), aov=gs.aov_kernel_name(), query=gs.query_kernel_name(),
                trace=gs.trace_kernel_name(), pixel=gs.pixel_kernel_name(), last=gs.last_launch_kernel(), status=gs.launch_status())


@refusal("launch_status", "failed")
def _(rec, names, kind):
    rec.answers["rt_hip_launch_status"] = -3
    stub(rec, names).launch_status()


# ---- readers -------------------------------------------------------------------------------------------------------------------------------------------
READERS = ("hull_facets", "bvh_info", "bvh_read", "bvh_cost", "rebuild_bvh", "rebuild_info", "read_spheres", "sphere_bounds", "read_triangles",
           "bounds", "update_info", "spheres")


@case("reader", *READERS, *(f"{r}_empty" for r in ("bvh_read", "read_spheres", "read_triangles", "spheres")), "spheres_twice", "bvh_read_nodes")
def _(rec, names, kind):
    empty = kind.endswith("_empty")
    gs = stub(rec, names, n_objects=0 if empty else 2, n_triangles=0 if empty else 3)
    if kind == "bvh_read_nodes":
        rec.effects["rt_hip_scene_bvh_info"] = lambda h, b, d, md, nn, cost: setattr(nn._obj, "value", 5)
    if kind == "spheres_twice":
        first = gs.spheres()
        return dict(same=gs.spheres() is first, values=first.tolist(), held=gs._spheres is first)
    return getattr(gs, kind[:-6] if empty else kind.replace("_nodes", ""))()


@case("maintain_bvh", "ratio", "integer")
def _(rec, names, kind):
    return stub(rec, names).maintain_bvh(1.5 if kind == "ratio" else 2)


# ---- updates -------------------------------------------------------------------------------------------------------------------------------------------
UPDATES = dict(update_vertices=((3, 3, 3), "n_triangles"), update_spheres=((2, 4), "n_objects"))
UPDATE_KINDS = ("tensor", "strided", "on_device", "array", "list", "float32_array")


def _update_input(names, shape, kind):
    if kind in ("tensor", "strided", "on_device"):
        t = torch.arange(int(np.prod(shape)), dtype=F64).reshape(shape)
        if kind == "strided":
            t = torch.stack([t, t], dim=-1)[..., 0]
        return names.add("input", t.as_subclass(OnDevice) if kind == "on_device" else t)
    a = np.arange(int(np.prod(shape)), dtype=np.float32 if kind == "float32_array" else np.float64).reshape(shape)
    return a.tolist() if kind == "list" else names.add("input", a)


for _m, (_shape, _) in UPDATES.items():
    @case(_m, *UPDATE_KINDS, "rebuild_above")
    def _(rec, names, kind, m=_m, shape=_shape):
        gs = stub(rec, names)
        x = _update_input(names, shape, "tensor" if kind == "rebuild_above" else kind)
        ret = getattr(gs, m)(x, **(dict(rebuild_above=1.25) if kind == "rebuild_above" and m == "update_vertices" else {}))
        held = getattr(gs, "_spheres", None)
        return dict(returns=ret, spheres=None if held is None else dict(
            what=names.describe(held), is_the_input=held is x, values=held.tolist(), plain=type(held) is torch.Tensor))

    @refusal(_m, "tensor_dtype", "tensor_shape", "tensor_both", "array_shape", "list_shape")
    def _(rec, names, kind, m=_m, shape=_shape):
        x = dict(tensor_dtype=z(*shape), tensor_shape=z(*shape[:-1], 5, dtype=F64), tensor_both=z(7), array_shape=np.zeros(shape[:-1] + (5,)),
                 list_shape=[[0.0] * 4] * 5)[kind]
        getattr(stub(rec, names), m)(x)


# ---- ray calls ---------------------------------------------------------------------------------------------------------------------------------------
def _rays(names, per_ray, kind):
    n = 0 if "n0" in kind else 3
    if "off16" in kind:
        return names.add("rays", off16(n, per_ray))
    if "listed" in kind:
        return [[0.25] * per_ray] * n
    return names.add("rays", z(n, per_ray, dtype=F64))


QUERY_KINDS = ("n3", "n0", "n3_tmax", "n0_tmax", "n3_tmax_listed", "n3_want_two", "n3_normalize_radius", "n3_off16", "n3_listed", "n0_want_two")


def _query_kw(names, kind):
    n = 0 if "n0" in kind else 3
    kw = {}
    if "tmax" in kind:
        kw["t_max"] = [1.0, 2.0, 3.0][:n] if "listed" in kind else names.add("t_max", z(n, dtype=F64))
    if "want_two" in kind:
        kw["want"] = ("t", "status")
    if "normalize_radius" in kind:
        kw.update(normalize=True, origin_radius=12.5)
    return kw


@case("query_rays", *QUERY_KINDS)
def _(rec, names, kind):
    gs = stub(rec, names)
    out = gs.query_rays(_rays(names, 6, kind), **_query_kw(names, kind))
    return dict(out=out, kept=gs._query_inputs)


def _far_camera(names):
    cam = names.add("camera", abi.Camera())
    cam.position.x, cam.position.y, cam.position.z = 3.0, 4.0, 12.0
    return cam


@case("query_uv", *QUERY_KINDS, "n3_camera", "n3_camera_radius", "n3_out_partly", "n3_out_all", "n3_out_beyond_want")
def _(rec, names, kind):
    gs = stub(rec, names)
    kw = _query_kw(names, kind)
    if "camera" in kind:
        kw["camera"] = _far_camera(names)
    if "camera_radius" in kind:
        kw["origin_radius"] = 0.5
    if "out_partly" in kind:
        kw["out"] = names.add("out", dict(t=z(3, dtype=F64), point=z(3, 3, dtype=F64)))
    if "out_all" in kind or "out_beyond" in kind:
        kw["out"] = names.add("out", {f: z(*((3, k) if k > 1 else (3,)), dtype=gpu._TORCH[d]) for f, (d, k) in abi.HIT_SHAPES.items()})
    if "out_beyond" in kind:
        kw["want"] = ("status", "t")
    out = gs.query_uv(_rays(names, 2, kind), **kw)
    return dict(out=out, kept=gs._query_inputs)


@refusal("query", "rays_tmax_count", "uv_tmax_count", "uv_out_shape", "uv_out_dtype", "uv_out_strided", "first_tmax_then_out", "rays_tmax_n0")
def _(rec, names, kind):
    gs = stub(rec, names)
    if kind == "rays_tmax_count":
        gs.query_rays(z(3, 6, dtype=F64), t_max=[1.0, 2.0])
    if kind == "rays_tmax_n0":
        gs.query_rays(z(0, 6, dtype=F64), t_max=[1.0])
    if kind == "uv_tmax_count":
        gs.query_uv(z(3, 2, dtype=F64), t_max=z(4, dtype=F64))
    out = dict(uv_out_shape=dict(point=z(3, dtype=F64)), uv_out_dtype=dict(t=z(3)), uv_out_strided=dict(t=strided(z(3, dtype=F64))),
               first_tmax_then_out=dict(t=z(3)))[kind]
    gs.query_uv(z(3, 2, dtype=F64), t_max=[1.0] if kind == "first_tmax_then_out" else None, out=out)


TRACE_KINDS = ("n3", "n0", "n3_stats", "n0_stats", "n3_depth", "n3_depth_0", "n3_everything", "n0_everything", "n3_normalize_radius_first", "n3_off16",
               "n3_listed")


def _trace_kw(names, kind, fields):
    kw = {}
    if "stats" in kind:
        kw["stats"] = names.add("stats", z(4, dtype=I64))
    if "depth" in kind:
        kw["max_depth"] = 0 if "depth_0" in kind else 2
    if "everything" in kind:
        kw["want"] = fields
    if "normalize_radius_first" in kind:
        kw.update(normalize=True, origin_radius=12.5, index_first=40)
    return kw


@case("trace_rays", *TRACE_KINDS)
def _(rec, names, kind):
    gs = stub(rec, names)
    out = gs.trace_rays(_rays(names, 6, kind), 2, 7, **_trace_kw(names, kind, abi.RADIANCE_FIELDS))
    return dict(out=out, kept=gs._trace_inputs)


@case("trace_uv", *TRACE_KINDS, "n3_camera", "n3_camera_radius")
def _(rec, names, kind):
    gs = stub(rec, names)
    kw = _trace_kw(names, kind, abi.RADIANCE_FIELDS)
    if "camera" in kind:
        kw["camera"] = _far_camera(names)
    if "camera_radius" in kind:
        kw["origin_radius"] = 0.5
    out = gs.trace_uv(_rays(names, 2, kind), 2, 7, **kw)
    return dict(out=out, kept=gs._trace_inputs)


@case("trace_pixels", "tensor", "listed", "empty", "empty_listed", "n_inside", "n_end", "n_0", "camera_depth_first", "depth_0", "stats", "everything",
      "strided_tensor")
def _(rec, names, kind):
    gs = stub(rec, names)
    pixels = names.add("pixels", z(3, dtype=I32))
    kw = {}
    if kind == "listed":
        pixels = [7, 3, 44]
    if kind == "empty":
        pixels = z(0, dtype=I32)
    if kind == "empty_listed":
        pixels = []
    if kind == "strided_tensor":
        pixels = names.add("pixels", strided(z(3, dtype=I32)))
    if kind.startswith("n_"):
        kw["n"] = dict(n_inside=2, n_end=3, n_0=0)[kind]
    if kind == "camera_depth_first":
        kw.update(camera=names.add("camera", abi.Camera()), max_depth=2, sample_first=6)
    if kind == "depth_0":
        kw["max_depth"] = 0
    if kind == "stats":
        kw["stats"] = names.add("stats", z(4, dtype=I64))
    if kind == "everything":
        kw["want"] = abi.PIXEL_FIELDS
    out = gs.trace_pixels(pixels, 2, 7, **kw)
    return dict(out=out, kept=gs._pixel_inputs)


@refusal("trace_pixels", "n_beyond", "n_negative", "want_ray", "want_stranger", "first_n_then_want", "float_pixels", "long_pixels",
         "first_pixels_then_n")
def _(rec, names, kind):
    gs = stub(rec, names)
    pixels = dict(float_pixels=z(3), long_pixels=z(3, dtype=I64), first_pixels_then_n=z(3)).get(kind, z(3, dtype=I32))
    n = dict(n_beyond=4, n_negative=-1, first_n_then_want=4, first_pixels_then_n=9).get(kind)
    want = dict(want_ray=("status", "ray"), want_stranger=("depth",), first_n_then_want=("ray",)).get(kind, ("status",))
    gs.trace_pixels(pixels, 2, 7, n=n, want=want)


def _answer_query(status, t):
    """an effect of rt_hip_query_rays: the first ray's status and t, and zeros in the other wanted fields (the wrapper's are torch.empty)"""
    def effect(handle, rays, t_max, n, params, hits, stream):
        for f, (dtype, k) in abi.HIT_SHAPES.items():
            if getattr(hits._obj, f):
                C.memset(getattr(hits._obj, f), 0, n * k * np.dtype(dtype).itemsize)
        C.c_uint32.from_address(hits._obj.status).value = status
        C.c_double.from_address(hits._obj.t).value = t
    return effect


@case("pick", "miss", "hit")
def _(rec, names, kind):
    rec.effects["rt_hip_query_rays"] = _answer_query(*((1, 6.0) if kind == "hit" else (0, 0.0)))
    return stub(rec, names).pick(4, 2)


@case("focus_at", "miss", "hit", "hit_camera")
def _(rec, names, kind):
    gs = stub(rec, names)
    cam = None
    rec.effects["rt_hip_query_rays"] = _answer_query(*((0, 0.0) if kind == "miss" else (1, 6.0)))
    if kind != "miss":
        gs.scene.camera.lower_left_corner.z = 3.0   # d = (0, 0, -3) on the scene's own camera
    if kind == "hit_camera":
        cam = names.add("camera", abi.Camera())
        cam.position.x, cam.horizontal.x, cam.vertical.y, cam.lower_left_corner.z = 1.0, 2.0, 4.0, -2.0
    return gs.focus_at(4, 2, camera=cam)


@case("refine", "count_0", "count_2", "count_2_all")
def _(rec, names, kind):
    gs = stub(rec, names)
    if kind != "count_0":
        rec.effects["rt_hip_select_pixels"] = plant(lambda *a: a[9].value, C.c_uint32, 2)
    rgb, values = names.add("rgb", z(H, W, 3)), names.add("values", z(H, W))
    kw = {}
    if kind == "count_2_all":
        kw = dict(sample_first=3, prior=names.add("prior", z(H, W)), prior_scale=2.0, invert=True, camera=names.add("camera", abi.Camera()),
                  max_depth=1, rgb8=names.add("rgb8", z(H, W, 3, dtype=U8)), weight=names.add("weight", z(H, W)), stats=names.add("stats", z(4, dtype=I64)))
    return gs.refine(rgb, values, 0.25, 0.75, 2, 7, **kw)


@case("render_panorama", "defaults", "depth")
def _(rec, names, kind):
    return stub(rec, names).render_panorama(4, 2, (3.0, 4.0, 12.0), 2, 7, **(dict(max_depth=1) if kind == "depth" else {}))


# ---- lens and probes -----------------------------------------------------------------------------------------------------------------------------------
@case("render_lens", "defaults", "slice", "camera_depth_stats", "depth_0")
def _(rec, names, kind):
    gs = stub(rec, names)
    kw = dict(defaults={}, slice=dict(slice_pixels=16), depth_0=dict(max_depth=0),
              camera_depth_stats=dict(camera=names.add("camera", abi.Camera()), max_depth=2, stats=names.add("stats", z(4, dtype=I64))))[kind]
    out = gs.render_lens(0.25, 6.0, 2, 7, **kw)
    return dict(out=out, kept=gs._lens_workspace)


BAKE_KINDS = ("plain", "details", "slice", "slice_beyond", "empty", "radius", "depth_stats", "depth_0", "listed", "not_finite")


def _bake_kw(names, kind):
    return dict(details=dict(details=True), slice=dict(slice_rays=4), slice_beyond=dict(slice_rays=1000), radius=dict(origin_radius=12.5),
                depth_stats=dict(max_depth=2, stats=names.add("stats", z(4, dtype=I64)), details=True), depth_0=dict(max_depth=0)).get(kind, {})


def _probe_positions(names, kind, name="positions"):
    if kind == "empty":
        return names.add(name, z(0, 3, dtype=F64))
    if kind == "listed":
        return [[3.0, 4.0, 12.0], [0.0, 0.0, 1.0]]
    t = torch.tensor([[3.0, 4.0, 12.0], [0.0, 0.0, 1.0]], dtype=F64)
    if kind == "not_finite":
        t[0, 0] = float("inf")
    return names.add(name, t)


@case("bake_probes", *BAKE_KINDS)
def _(rec, names, kind):
    gs = stub(rec, names)
    out = gs.bake_probes(_probe_positions(names, kind), 3, 7, **_bake_kw(names, kind))
    return dict(out=out, kept=gs._probe_buffers)


@case("bake_irradiance", *BAKE_KINDS, "bias", "bias_radius")
def _(rec, names, kind):
    gs = stub(rec, names)
    kw = _bake_kw(names, kind)
    if "bias" in kind:
        kw["bias"] = 0.5
    if kind == "bias_radius":
        kw["origin_radius"] = 12.5
    pos = _probe_positions(names, kind)
    nrm = [[0.0, 2.0, 0.0], [0.0, 0.0, 1.0]] if kind == "listed" else names.add("normals", z(0 if kind == "empty" else 2, 3, dtype=F64) + 2.0)
    out = gs.bake_irradiance(pos, nrm, 3, 7, **kw)
    return dict(out=out, kept=gs._probe_buffers)


@refusal("bake_irradiance", "normals_count", "no_normals_for_some", "some_normals_for_none")
def _(rec, names, kind):
    n, m = dict(normals_count=(2, 3), no_normals_for_some=(2, 0), some_normals_for_none=(0, 1))[kind]
    stub(rec, names).bake_irradiance(z(n, 3, dtype=F64), z(m, 3, dtype=F64), 3, 7)


@case("bake_probe_grid", "plain", "details", "slice", "slice_beyond", "empty", "radius", "depth_stats", "depth_0")
def _(rec, names, kind):
    gs = stub(rec, names)
    out = gs.bake_probe_grid(grid((2, 0, 2)) if kind == "empty" else grid(), 3, 7, **_bake_kw(names, kind))
    return dict(out=out, kept=gs._probe_buffers)


@case("probe_preview", "defaults", "given", "listed", "strided")
def _(rec, names, kind):
    gs = stub(rec, names)
    coeff = names.add("coeff", z(4, 9, 3, dtype=F64))
    kw = dict(camera=names.add("camera", abi.Camera()), aov_samples=2, seed=9) if kind == "given" else {}
    if kind == "listed":
        coeff = [0.5] * (4 * 27)
    if kind == "strided":
        coeff = names.add("coeff", strided(z(4, 9, 3, dtype=F64)))
    out = gs.probe_preview(grid(), coeff, **kw)
    return dict(out=out, kept=gs._preview_buffers)


@refusal("probe_preview", "coeff_count", "coeff_for_an_empty_grid")
def _(rec, names, kind):
    stub(rec, names).probe_preview(grid() if kind == "coeff_count" else grid((2, 0, 2)), z(3, 9, 3, dtype=F64))


@case("lens_rays", "whole", "part", "n0", "negative")
def _(rec, names, kind):
    cam = names.add("camera", abi.Camera())
    kw = dict(whole={}, part=dict(pixel_first=5, n=7, device=2), n0=dict(pixel_first=W * H), negative=dict(pixel_first=W * H + 2))[kind]
    return gpu.lens_rays(cam, W, H, 0.25, 6.0, 7, 1, **kw)


@case("lens_resolve", "plain", "strided", "empty")
def _(rec, names, kind):
    total = names.add("total", z(H, W, 3, dtype=F64))
    if kind == "strided":
        total = names.add("total", strided(z(H, W, 3, dtype=F64)))
    if kind == "empty":
        total = z(0, W, 3, dtype=F64)
    return gpu.lens_resolve(total, 2)


@case("probe_rays", "sphere", "hemisphere", "part", "n0", "empty", "listed", "negative")
def _(rec, names, kind):
    pos = _probe_positions(names, kind if kind in ("empty", "listed") else "plain")
    kw = dict(hemisphere=dict(normals=names.add("normals", z(2, 3, dtype=F64)), bias=0.5), part=dict(k_first=2, n=3, device=2), n0=dict(k_first=6),
              listed=dict(normals=[[0.0, 1.0, 0.0]] * 2), negative=dict(k_first=8)).get(kind, {})
    return gpu.probe_rays(pos, 3, 7, **kw)


@case("probe_resolve", "sphere", "hemisphere", "empty", "strided")
def _(rec, names, kind):
    total = names.add("total", z(2, 1 if kind == "hemisphere" else 9, 3, dtype=F64))
    if kind == "empty":
        total = z(0, 9, 3, dtype=F64)
    if kind == "strided":
        total = names.add("total", strided(z(2, 9, 3, dtype=F64)))
    return gpu.probe_resolve(total, 3)


@case("probe_irradiance", "m3", "m0", "no_probes", "listed", "long_index", "strided_sh")
def _(rec, names, kind):
    sh = names.add("sh", z(0 if kind == "no_probes" else 2, 9, 3, dtype=F64))
    m = 0 if kind == "m0" else 3
    index, normals = names.add("index", z(m, dtype=I32)), names.add("normals", z(m, 3, dtype=F64))
    if kind == "listed":
        index, normals = [0, 1, 5], [[0.0, 1.0, 0.0]] * 3
    if kind == "long_index":
        index = names.add("index", torch.tensor([0, -1, 2 ** 32 + 1], dtype=I64))
    if kind == "strided_sh":
        sh = names.add("sh", strided(z(2, 9, 3, dtype=F64)))
    return gpu.probe_irradiance(sh, index, normals)


@refusal("probe_irradiance", "index_count", "no_index")
def _(rec, names, kind):
    gpu.probe_irradiance(z(2, 9, 3, dtype=F64), [0, 1] if kind == "index_count" else [], z(3, 3, dtype=F64))


@case("probe_grid_positions", "plain", "empty", "device")
def _(rec, names, kind):
    return gpu.probe_grid_positions(grid((2, 0, 2)) if kind == "empty" else grid(), **(dict(device=2) if kind == "device" else {}))


SHADE_KINDS = ("plain", "m0", "status_int32", "status_long", "status_listed", "albedo_add", "want_irradiance", "want_color", "out_both", "out_one",
               "out_not_wanted", "first_two", "listed", "strided_coeff")


@case("probe_shade", *SHADE_KINDS)
def _(rec, names, kind):
    n = 0 if kind == "m0" else 3
    coeff, pts, nrm = names.add("coeff", z(4, 9, 3, dtype=F64)), names.add("points", z(n, 3, dtype=F64)), names.add("normals", z(n, 3, dtype=F64))
    kw = {}
    if kind == "status_int32":
        kw["status"] = names.add("status", z(3, dtype=I32))
    if kind == "status_long":
        kw["status"] = names.add("status", z(3, dtype=I64))
    if kind == "status_listed":
        kw["status"] = [1, 0, 2]
    if kind == "albedo_add":
        kw.update(albedo=names.add("albedo", z(3, 3)), add=names.add("add", z(3, 3)), status=names.add("status", z(3, dtype=I32)))
    if kind.startswith("want_"):
        kw["want"] = (kind[5:],)
    if kind == "out_both":
        kw["out"] = names.add("out", dict(irradiance=z(3, 3, dtype=F64), color=z(3, 3)))
    if kind == "out_one":
        kw["out"] = names.add("out", dict(color=z(3, 3)))
    if kind == "out_not_wanted":
        kw.update(out=names.add("out", dict(irradiance=z(3, 3, dtype=F64), color=z(3, 3))), want=("color",))
    if kind == "first_two":
        kw["m"] = 2
    if kind == "listed":
        pts, nrm = [[0.0, 1.0, 2.0]] * 3, [[0.0, 1.0, 0.0]] * 3
        kw.update(albedo=[[0.5] * 3] * 3, add=[[0.25] * 3] * 3)
    if kind == "strided_coeff":
        coeff = names.add("coeff", strided(z(4, 9, 3, dtype=F64)))
    return gpu.probe_shade(grid(), coeff, pts, nrm, **kw)


@refusal("probe_shade", "normals_count", "status_count", "albedo_count", "add_count", "first_normals_then_status", "first_status_then_albedo",
         "first_albedo_then_add")
def _(rec, names, kind):
    nrm = z(2 if "normals" in kind else 3, 3, dtype=F64)
    status = z(2, dtype=I32) if "status" in kind else None
    albedo = z(2, 3) if "albedo" in kind else None
    add = z(4, 3) if "add" in kind else None
    gpu.probe_shade(grid(), z(4, 9, 3, dtype=F64), z(3, 3, dtype=F64), nrm, status=status, albedo=albedo, add=add)


# ---- the rest of Accumulation --------------------------------------------------------------------------------------------------------------------------
def _accum(rec, names, count=2, **kw):
    gs = stub(rec, names)
    acc = gpu.Accumulation(gs, names.add("accum", C.c_void_p(ACCUM)), count, seed=7, **kw)
    names.keep.append(acc)
    return gs, acc


@case("accumulation", "properties", "tile_samples", "run_adaptive", "run_adaptive_params", "run_adaptive_callback", "close", "close_twice")
def _(rec, names, kind):
    gs, acc = _accum(rec, names)
    if kind == "properties":
        rec.answers.update(rt_hip_accum_samples=3, rt_hip_accum_live_tiles=2)
        return dict(samples=acc.samples, kernel=acc.kernel, live_tiles=acc.live_tiles)
    if kind == "tile_samples":
        return acc.tile_samples()
    if kind.startswith("run_adaptive"):
        seen = []
        if kind == "run_adaptive_callback":
            def effect(handle, p, stats, secs, cb, user):
                fn = C.cast(cb, abi.ADAPT_CHECKPOINT)
                seen.append([fn(None, 4, 2), fn(None, 8, 0)])
            rec.effects["rt_hip_accum_run_adaptive"] = effect
        kw = dict(run_adaptive={}, run_adaptive_params=dict(min_samples=2, threshold=0.5, dilate=0),
                  run_adaptive_callback=dict(on_checkpoint=lambda done, live: seen.append((done, live)) or live == 0))[kind]
        return dict(returns=acc.run_adaptive(**kw), seen=seen)
    gs._accums = [acc.handle]
    acc.close()
    if kind == "close_twice":
        acc.close()
    return dict(handle=acc.handle.value, the_scenes=gs._accums[0].value)


@case("freeze", "error", "error_params", "mask_list", "mask_array", "mask_tensor", "mask_bools", "mask_2d")
def _(rec, names, kind):
    gs, acc = _accum(rec, names, count=4)
    rec.effects["rt_hip_accum_freeze"] = lambda h, e, t, d, live, s: setattr(live._obj, "value", 3)
    rec.effects["rt_hip_accum_freeze_mask"] = lambda h, m, live, s: setattr(live._obj, "value", 1)
    if kind.startswith("error"):
        return acc.freeze(error=names.add("error", z(4)), **(dict(threshold=0.5, dilate=2) if kind == "error_params" else {}))
    mask = dict(mask_list=[1, 0, 2, 0], mask_array=np.array([1, 0, 2, 0], np.int64), mask_tensor=torch.tensor([1.5, 0.0, 2.0, 0.0]),
                mask_bools=[True, False, True, False], mask_2d=np.array([[1, 0], [2, 0]]))[kind]
    return acc.freeze(mask=names.add("mask", mask))


@refusal("freeze", "neither", "both", "error_dtype", "error_count", "error_strided", "mask_count", "first_both_then_error", "bad_threshold_then_error")
def _(rec, names, kind):
    gs, acc = _accum(rec, names, count=4)
    kw = dict(neither={}, both=dict(error=z(4), mask=[1] * 4), error_dtype=dict(error=z(4, dtype=F64)), error_count=dict(error=z(5)),
              error_strided=dict(error=strided(z(4))), mask_count=dict(mask=[1] * 5), first_both_then_error=dict(error=z(5), mask=[1] * 5),
              bad_threshold_then_error=dict(error=z(5), threshold="much"))[kind]
    try:
        acc.freeze(**kw)
    except TypeError as e:   # (the parameter builder's own complaint comes before the tensor's refusal)
        raise ValueError("TypeError first: %s" % e)


@refusal("denoised", "part_of_the_image", "no_samples", "first_part_then_samples")
def _(rec, names, kind):
    gs, acc = _accum(rec, names, count=1 if "part" in kind else gpu.n_tiles(W, H))
    rec.answers["rt_hip_accum_samples"] = 0 if "samples" in kind else 2
    acc.denoised()


@case("denoised", "plain", "camera_params")
def _(rec, names, kind):
    gs, acc = _accum(rec, names, count=gpu.n_tiles(W, H), **(dict(camera=names.add("camera", abi.Camera())) if kind == "camera_params" else {}))
    rec.answers["rt_hip_accum_samples"] = 3
    return acc.denoised(**(dict(iterations=2, demodulate=True) if kind == "camera_params" else {}))


# ---- composites ------------------------------------------------------------------------------------------------------------------------------------------
@case("render_image", "defaults", "given", "whitted", "chunks_2")
def _(rec, names, kind):
    gs = stub(rec, names)
    if kind == "chunks_2":
        rec.answers["rt_hip_suggest_chunks_depth"] = 2
    kw = dict(given=dict(samples=2, max_depth=0), whitted=dict(integrator="whitted")).get(kind, {})
    out = gs.render_image(7, **kw)
    return dict(out=out, workspace=gs._workspace)


@case("aov_image", "plain")
def _(rec, names, kind):
    return stub(rec, names).aov_image(7, 2)


@case("denoised_image", "plain", "params")
def _(rec, names, kind):
    return stub(rec, names).denoised_image(7, 2, **(dict(iterations=2, object_edges=True) if kind == "params" else {}))


@case("render_adaptive", "defaults", "given")
def _(rec, names, kind):
    gs = stub(rec, names)
    kw = dict(max_depth=0, integrator="whitted", min_samples=2, threshold=0.5) if kind == "given" else {}
    out = gs.render_adaptive(7, 4, **kw)
    return dict(out=out, accums=[h.value for h in gs._accums])


@refusal("render_adaptive", "failed_run")
def _(rec, names, kind):
    rec.answers["rt_hip_accum_run_adaptive"] = -2
    gs = stub(rec, names)
    try:
        gs.render_adaptive(7, 4)
    finally:
        assert [h.value for h in gs._accums] == [None]   # closed on the way out


def _preview(rec, names, scale=2, **params):
    gs = stub(rec, names)
    gs.device = 2
    pv = gpu.Preview(gs, scale, **params)
    names.keep.append(pv)
    return gs, pv


@case("preview", "init", "init_params", "frame", "frame_camera_denoise", "frame_fill", "frame_fill_2", "close", "through_the_scene")
def _(rec, names, kind):
    if kind == "through_the_scene":
        gs = stub(rec, names)
        pv = names.add("preview", gs.preview(3, sigma_depth=0.25))
        names.keep.append(pv)
        return dict(scale=pv.scale, params=pv.params, low=[pv.low_width, pv.low_height])
    gs, pv = _preview(rec, names, **(dict(sigma_depth=0.25, demodulate=True) if kind == "init_params" else {}))
    if kind.startswith("init"):
        low = pv.low.scene
        return dict(scale=pv.scale, params=pv.params, low=[pv.low_width, pv.low_height], low_scene=[low.width, low.height, low.samples, low.max_depth],
                    same_camera=low.camera is gs.scene.camera, same_objects=low.objects is gs.scene.objects, device=pv.low.device,
                    handle=names[pv.low.handle.value])
    if kind == "close":
        pv.close()
        return dict(low_handle=pv.low.handle, handle=names[gs.handle.value])
    if kind == "frame_fill_2":
        rec.effects["rt_hip_select_pixels"] = plant(lambda *a: a[9].value, C.c_uint32, 2)
    kw = dict(frame={}, frame_camera_denoise=dict(camera=names.add("camera", abi.Camera()), denoise=True, iterations=2), frame_fill=dict(fill=2),
              frame_fill_2=dict(fill=2.0, camera=names.add("camera", abi.Camera())))[kind]
    return pv.frame(7, 2, **kw)


@refusal("preview", "scale_1", "scale_fraction", "low_too_small", "bad_keyword", "first_scale_then_keyword", "fill_0", "fill_fraction",
         "fill_without_conf")
def _(rec, names, kind):
    if kind in ("fill_0", "fill_fraction", "fill_without_conf"):
        gs, pv = _preview(rec, names)
        if kind == "fill_without_conf":
            real = gpu.upsample
            gpu.upsample = lambda *a, **kw: {f: v for f, v in real(*a, **kw).items() if f != "conf"}
            try:
                pv.frame(7, 2, fill=1)
            finally:
                gpu.upsample = real
        pv.frame(7, 2, fill=0 if kind == "fill_0" else 1.5)
    scale = dict(scale_1=1, scale_fraction=2.5, low_too_small=5, bad_keyword=2, first_scale_then_keyword=1)[kind]
    try:
        gpu.Preview(stub(rec, names), scale, **(dict(sigma=1.0) if "keyword" in kind else {}))
    except TypeError as e:
        raise ValueError("TypeError: %s" % e)


# ---- host forms ------------------------------------------------------------------------------------------------------------------------------------------
HOST_KINDS = ("defaults", "camera", "depth", "depth_0", "camera_depth")


def _host_kw(names, kind, camera=True):
    kw = {}
    if "camera" in kind and camera:
        kw["camera"] = names.add("camera", abi.Camera())
    if "depth" in kind:
        kw["max_depth"] = 0 if kind == "depth_0" else 2
    return kw


@case("render_image_host", "defaults", "given", "depth_0", "samples_0")
def _(rec, names, kind):
    kw = dict(given=dict(n_devices=2, samples=9, max_depth=2, integrator="whitted"), depth_0=dict(max_depth=0), samples_0=dict(samples=0)).get(kind, {})
    return gpu.render_image_host(host_scene(names), 7, **kw)


@case("adaptive_image_host", "defaults", "given", "depth_0")
def _(rec, names, kind):
    kw = dict(given=dict(device=3, max_depth=2, integrator="whitted", min_samples=2, threshold=0.5, dilate=0), depth_0=dict(max_depth=0)).get(kind, {})
    return gpu.adaptive_image_host(host_scene(names), 7, 4, **kw)


@case("query_rays_host", "n3", "n0", "n3_tmax", "n0_tmax", "n3_camera", "n0_camera", "n3_want_two", "n3_normalize_radius_device", "n3_listed")
def _(rec, names, kind):
    n = 0 if "n0" in kind else 3
    kw = {}
    if "camera" in kind:
        kw["camera"] = _far_camera(names)
    rays = names.add("rays", np.full((n, 2 if "camera" in kind else 6), 0.5))
    if "listed" in kind:
        rays = [[0.25] * 6] * 3
    if "tmax" in kind:
        kw["t_max"] = names.add("t_max", np.full(n, 2.0))
    if "want_two" in kind:
        kw["want"] = ("t", "status")
    if "normalize" in kind:
        kw.update(normalize=True, origin_radius=12.5, device=3)
    return gpu.query_rays_host(host_scene(names), rays, **kw)


@refusal("query_rays_host", "tmax_count", "tmax_n0")
def _(rec, names, kind):
    gpu.query_rays_host(host_scene(names), np.zeros((3 if kind == "tmax_count" else 0, 6)), t_max=[1.0, 2.0])


@case("trace_rays_host", "n3", "n0", "n3_camera", "n0_camera", "n3_depth", "n3_depth_0", "n3_everything", "n3_normalize_radius_first_device", "n3_listed")
def _(rec, names, kind):
    n = 0 if "n0" in kind else 3
    kw = _host_kw(names, kind, camera=False)
    if "camera" in kind:
        kw["camera"] = _far_camera(names)
    rays = names.add("rays", np.full((n, 2 if "camera" in kind else 6), 0.5))
    if "listed" in kind:
        rays = [[0.25] * 6] * 3
    if "everything" in kind:
        kw["want"] = abi.RADIANCE_FIELDS
    if "normalize" in kind:
        kw.update(normalize=True, origin_radius=12.5, index_first=40, device=3)
    return gpu.trace_rays_host(host_scene(names), rays, 2, 7, **kw)


@case("trace_pixels_host", *HOST_KINDS, "empty", "everything_first_device", "converted")
def _(rec, names, kind):
    kw = _host_kw(names, kind)
    pixels = names.add("pixels", np.array([7, 3, 44], np.uint32))
    if kind == "empty":
        pixels = []
    if kind == "converted":
        pixels = names.add("pixels", np.array([[7, 3], [44, 1]], np.int64))
    if kind == "everything_first_device":
        kw.update(want=abi.PIXEL_FIELDS, sample_first=6, device=3)
    return gpu.trace_pixels_host(host_scene(names), pixels, 2, 7, **kw)


@case("render_lens_host", *HOST_KINDS, "device")
def _(rec, names, kind):
    return gpu.render_lens_host(host_scene(names), 0.25, 6.0, 2, 7, **_host_kw(names, kind), **(dict(device=3) if kind == "device" else {}))


@case("probe_preview_host", *HOST_KINDS, "radius_samples_device", "empty")
def _(rec, names, kind):
    kw = _host_kw(names, kind)
    if kind == "radius_samples_device":
        kw.update(origin_radius=12.5, aov_samples=2, device=3)
    return gpu.probe_preview_host(host_scene(names), grid((2, 0, 2)) if kind == "empty" else grid(), 3, 7, **kw)


@case("bake_probes_host", "sphere", "hemisphere", "hemisphere_bias", "depth", "depth_0", "radius_device", "empty", "listed", "not_finite", "converted")
def _(rec, names, kind):
    kw = _host_kw(names, kind)
    pos = names.add("positions", np.array([[3.0, 4.0, 12.0], [0.0, 0.0, 1.0]]))
    if "hemisphere" in kind:
        kw["normals"] = names.add("normals", np.full((2, 3), 2.0))
    if kind == "hemisphere_bias":
        kw["bias"] = 0.5
    if kind == "radius_device":
        kw.update(origin_radius=12.5, device=3)
    if kind == "empty":
        pos = np.zeros((0, 3))
    if kind == "listed":
        pos, kw["normals"] = pos.tolist(), [[0.0, 1.0, 0.0]] * 2
    if kind == "not_finite":
        pos[0, 0] = np.inf
    if kind == "converted":
        pos = names.add("positions", pos.astype(np.float32))
    return gpu.bake_probes_host(host_scene(names), pos, 3, 7, **kw)


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_recorded():
    g = _golden()
    assert sorted(g["transcripts"]) == sorted(T) and sorted(g["refusals"]) == sorted(R)


@pytest.mark.parametrize("case", sorted(T))
def test_transcript(monkeypatch, case):
    assert _transcript(monkeypatch, T[case]) == _golden()["transcripts"][case]


@pytest.mark.parametrize("case", sorted(R))
def test_refusal(monkeypatch, case):
    assert _refusal(monkeypatch, R[case]) == _golden()["refusals"][case]


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: test_scene_front_calls.py --record"
    recorded = dict(transcripts={}, refusals={})
    for name in sorted(T):
        with pytest.MonkeyPatch.context() as mp:
            recorded["transcripts"][name] = _transcript(mp, T[name])
    for name in sorted(R):
        with pytest.MonkeyPatch.context() as mp:
            recorded["refusals"][name] = _refusal(mp, R[name])
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(T)} transcripts, {len(R)} refusals -> {GOLDEN}")
