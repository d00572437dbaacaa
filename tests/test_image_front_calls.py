"""What the image-space wrappers of rt_amd/gpu.py hand to the shim, and what they refuse, pinned without a device and without a built
shim: abi.load_shim is replaced by a recorder, torch's current stream by a constant, and the wrappers are fed CPU tensors and numpy
arrays.  A transcript is the list of shim calls of one case -- symbol and arguments, every address replaced by the name of the buffer
it belongs to ("p:" a c_void_p, "i:" a plain int; "ret.*" a buffer the wrapper allocated and returned, "tmp" one it kept to itself,
"new:<first word>" an array a host form converted), records field by field -- and what the wrapper returned.  A refusal is the whole
text of the ValueError.  Both were recorded from the tree before the wrappers were folded (tests/golden/image_front_calls.json;
`python tests/test_image_front_calls.py --record` writes the file) and must not move.  The parameter builders of abi go through the
recorder as well: their records hold zeros plus what the case sets."""
import ctypes as C
import functools
import itertools
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(_root, "raytracer.c_amd"))

from rt_amd import abi, gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_front_calls.json")
STREAM = 0x57AEA300
SCENE = 0x5CE0E000
W, H = 9, 5
WL, HL = 5, 3
CPU = torch.device("cpu")
_BYREF = type(C.byref(C.c_int()))
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


# ---- the recorder ------------------------------------------------------------------------------------------------------------------------------
def _is_host(symbol):
    return symbol.endswith("_host") or symbol.endswith("_image")


def _raw_addresses(symbol, args):
    for a, ctype in zip(args, abi.SHIM_SYMBOLS[symbol][1]):
        if isinstance(a, _BYREF):
            a = a._obj
        if isinstance(a, (abi.RtHipAov, abi.RtHipHits)):
            for f, _ in a._fields_:
                yield getattr(a, f)
        elif ctype is C.c_void_p:
            yield a.value if isinstance(a, C.c_void_p) else a


class Recorder:
    """stands for the shim: every symbol records its call -- normalised at once, while the buffers behind the addresses are alive --
    and answers a small size for *_workspace_bytes and 0 otherwise"""

    def __init__(self, names=None):
        self.calls, self.names = [], names

    def __getattr__(self, symbol):
        def call(*args):
            words = {}
            if _is_host(symbol):   # the first word behind every address, while what a host form converted is still alive
                for v in _raw_addresses(symbol, args):
                    if v not in (None, 0, 1, STREAM):
                        words[v] = C.c_uint32.from_address(v).value
            if self.names is not None and symbol != "rt_hip_scene_destroy":   # (a stub scene's finaliser)
                self.calls.append(_normalise(self.names, symbol, args, words))
            return 64 if symbol.endswith("_workspace_bytes") else 0
        return call


class Names(dict):
    """address -> the name of the buffer there (the first name given wins); keeps what it names alive"""

    def __init__(self):
        super().__init__()
        self.keep = []

    def add(self, name, obj):
        self.keep.append(obj)
        if isinstance(obj, dict):
            for k, v in obj.items():
                self.add(f"{name}.{k}", v)
        elif isinstance(obj, (tuple, list)):
            for k, v in enumerate(obj):
                self.add(f"{name}[{k}]", v)
        elif isinstance(obj, torch.Tensor):
            if obj.numel() and obj.device == CPU:
                self.setdefault(obj.data_ptr(), name)
        elif isinstance(obj, np.ndarray):
            if obj.size:
                self.setdefault(obj.ctypes.data, name)
        elif isinstance(obj, abi.Camera):
            self.setdefault(C.addressof(obj), name)
        elif isinstance(obj, C.c_void_p):
            self.setdefault(obj.value, name)
        return obj

    def where(self, v, words, host):
        if v is None:
            return "NULL"
        if v == 1:
            return "1"
        if v == STREAM:
            return "stream"
        if v in self:
            return self[v]
        return "?%d:%s?" % (v, "new:%08x" % words[v] if host else "tmp")   # (settle(): a buffer the wrapper returns, or its own)

    def settle(self, calls, ret):
        """the addresses no name was known for at the call: "ret.*" where the wrapper returned the buffer, else "tmp" / "new:..."."""
        returned = Names()
        returned.add("ret", ret)
        for a, name in returned.items():
            self.setdefault(a, name)
        return json.loads(re.sub(r"\?(\d+):([^?]*)\?", lambda m: returned.get(int(m.group(1)), m.group(2)), json.dumps(calls)))

    def describe(self, r):
        if isinstance(r, dict):
            return {k: self.describe(v) for k, v in r.items()}
        if isinstance(r, (tuple, list)):
            return [self.describe(v) for v in r]
        if isinstance(r, torch.Tensor):
            return "%s %s %s" % (self.get(r.data_ptr(), "empty") if r.numel() else "empty", r.dtype, list(r.shape))
        if isinstance(r, np.ndarray):
            return "%s numpy.%s %s" % (self.get(r.ctypes.data, "empty") if r.size else "empty", r.dtype, list(r.shape))
        return r


def _normalise(names, symbol, args, words):
    host = _is_host(symbol)

    def field(v, ctype):
        if ctype is C.c_void_p:
            return None if v is None else names.where(v, words, host)
        if isinstance(v, C._Pointer):
            return "camera:" + names.get(C.addressof(v.contents), "?") if v else None
        return list(v) if isinstance(v, C.Array) else v

    out = []
    for a, ctype in zip(args, abi.SHIM_SYMBOLS[symbol][1]):
        if isinstance(a, _BYREF):
            a = a._obj
        if isinstance(a, abi.Camera):
            out.append("camera:" + names.get(C.addressof(a), "?"))
        elif isinstance(a, C.Structure):
            out.append(dict([("record", type(a).__name__)] + [(f, field(getattr(a, f), t)) for f, t in a._fields_]))
        elif ctype is C.c_void_p and a is not None:
            out.append("p:" + names.where(a.value, words, host) if isinstance(a, C.c_void_p) else "i:" + names.where(a, words, host))
        else:
            out.append(a)
    assert len(args) == len(abi.SHIM_SYMBOLS[symbol][1]), symbol
    return [symbol, out]


def _patch(mp, rec):
    mp.setattr(abi, "load_shim", lambda: rec)
    mp.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=STREAM))
    mp.setattr(torch, "device", lambda *a: CPU)   # what a scene allocates "on its device" lands on the host


def _transcript(mp, fn):
    names = Names()
    rec = Recorder(names)
    _patch(mp, rec)
    ret = fn(rec, names)
    calls = names.settle(rec.calls, ret)
    return json.loads(json.dumps(dict(calls=calls, returns=names.describe(ret))))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def z(*shape, dtype=F32):
    return torch.zeros(shape, dtype=dtype)


def aov_t(w, h):
    return dict(albedo=z(h, w, 3), normal=z(h, w, 3), depth=z(h, w), object=z(h, w, dtype=I32), hits=z(h, w, dtype=I32))


def aov_np(w, h, dtype=None):
    """as GpuScene.aov_image gives them (dtype: every field as that one instead, for the host forms to convert)"""
    a = dict(albedo=np.full((h, w, 3), 1.0, np.float32), normal=np.full((h, w, 3), 2.0, np.float32), depth=np.full((h, w), 3.0, np.float32),
             object=np.full((h, w), 4, np.uint32), hits=np.full((h, w), 5, np.uint32))
    return a if dtype is None else {f: v.astype(dtype) for f, v in a.items()}


def hits_t(n, moved=True):
    h = dict(status=z(n, dtype=I32), prim=z(n, dtype=I32), object=z(n, dtype=I32), bary=z(n, 2, dtype=F64), point=z(n, 3, dtype=F64))
    return h if moved else {f: v for f, v in h.items() if f != "object"}


def hits_np(n, moved=True, dtype=None):
    h = dict(status=np.full(n, 1, np.uint32), prim=np.full(n, 2, np.uint32), object=np.full(n, 3, np.uint32),
             bary=np.full((n, 2), 4.0), point=np.full((n, 3), 5.0))
    h = h if moved else {f: v for f, v in h.items() if f != "object"}
    return h if dtype is None else {f: v.astype(dtype) for f, v in h.items()}


def meta(t):
    return torch.empty_like(t, device="meta")


def strided(t):
    """a tensor of t's shape and dtype that is not contiguous"""
    return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]


def scene_stub(rec, names, w=W, h=H):
    gs = object.__new__(gpu.GpuScene)
    gs.shim, gs.device, gs._accums = rec, 0, []
    gs.scene = types.SimpleNamespace(width=w, height=h, samples=4, max_depth=5, camera=names.add("scene.camera", abi.Camera()))
    gs.handle = names.add("scene", C.c_void_p(SCENE))
    return gs


# ---- (a) the transcripts -------------------------------------------------------------------------------------------------------------------------
T = {}


def _tile_error(kind):
    def run(rec, names):
        count = 1 if kind == "subset" else 2
        cur, prev = names.add("cur", z(count, 64, 3)), names.add("prev", z(count, 64, 3))
        kw = dict(first=1, stride=2, count=1) if kind == "subset" else {}
        if kind == "out":
            kw["out"] = names.add("out", z(2))
        return gpu.tile_error(cur, prev, W, H, **kw)
    return run


for _k in ("plain", "subset", "out"):
    T[f"tile_error-{_k}"] = _tile_error(_k)


def _denoise(kind):
    def run(rec, names):
        rgb, aov = names.add("rgb", z(H, W, 3)), names.add("aov", aov_t(W, H))
        kw = {}
        if kind == "in_place":
            kw["out"] = rgb
        if kind == "out":
            kw["out"] = names.add("out", z(H * W * 3))
        if kind == "params":
            kw.update(iterations=3, sigma_color=0.5, demodulate=True, object_edges=True)
        if kind == "needed_only":
            aov = {f: aov[f] for f in ("normal", "depth", "hits")}
        if kind == "stranger":   # a key that is no field of the record: checked with the rest, not packed
            aov = dict(aov, variance=names.add("variance", z(H, W)))
        return gpu.denoise(rgb, aov, W, H, **kw)
    return run


for _k in ("plain", "in_place", "out", "params", "needed_only", "stranger"):
    T[f"denoise-{_k}"] = _denoise(_k)


def _select(kind):
    def run(rec, names):
        values = names.add("values", z(H, W))
        kw = dict(none={}, zero=dict(capacity=0), four=dict(capacity=4), invert=dict(invert=True),
                  indices=dict(indices=names.add("indices", z(50, dtype=I32))),
                  four_indices=dict(capacity=4, indices=names.add("indices4", z(6, dtype=I32))),
                  zero_indices=dict(capacity=0, indices=names.add("indices0", z(6, dtype=I32))))[kind]
        return gpu.select_pixels(values, W, H, 0.25, 0.75, **kw)
    return run


for _k in ("none", "zero", "four", "invert", "indices", "four_indices", "zero_indices"):
    T[f"select_pixels-capacity_{_k}"] = _select(_k)


def _blend(kind):
    def run(rec, names):
        n = 0 if kind == "empty" else 3
        pixels = names.add("pixels", z(n, dtype=I32))
        status, radiance, rgb = names.add("status", z(3, dtype=I32)), names.add("radiance", z(3, 3, dtype=F64)), names.add("rgb", z(H, W, 3))
        kw = {}
        if kind in ("all", "empty_all"):
            kw = dict(prior=names.add("prior", z(H, W)), rgb8=names.add("rgb8", z(H, W, 3, dtype=U8)), weight=names.add("weight", z(H, W)))
        if kind == "weight_is_prior":
            kw = dict(prior=names.add("prior", z(H, W)))
            kw["weight"] = kw["prior"]
        if kind in ("first_two", "empty_all"):
            kw["n"] = 2 if kind == "first_two" else 0
        if kind == "listed":   # anything numpy takes: a new tensor the wrapper keeps to itself
            pixels = [7, 3, 44]
        return gpu.blend_pixels(pixels, status, radiance, rgb, W, H, 4.0, 0.5, **kw)
    return run


for _k in ("plain", "empty", "all", "empty_all", "weight_is_prior", "first_two", "listed"):
    T[f"blend_pixels-{_k}"] = _blend(_k)


def _spheres(kind, make):
    if kind == "none":
        return None, None
    k = 0 if kind == "empty" else 2
    return make(k), make(k)


def _prev_points(moved, n, positions, spheres, out):
    def run(rec, names):
        hits = names.add("hits", hits_t(n, moved))
        pos = names.add("positions", z(2, 3, 3, dtype=F64)) if positions == "given" else None
        if positions == "strided":   # not refused: a contiguous copy goes down
            pos = names.add("positions", z(2, 3, 3, 2, dtype=F64))[..., 0]
        o = dict(none=None, given=names.add("out", z(n, 3, dtype=F64)), point=hits["point"])[out]
        if not moved:
            return gpu.prev_points(hits, pos, out=o)
        sp, sc = _spheres(spheres, lambda k: z(k, 4, dtype=F64))
        names.add("spheres_prev", sp), names.add("spheres_cur", sc)
        return gpu.prev_points_moved(hits, pos, sp, sc, out=o)
    return run


def _prev_points_host(moved, n, positions, spheres, dtype=None):
    def run(rec, names):
        hits = names.add("hits", hits_np(n, moved, dtype))
        pos = names.add("positions", np.full((2, 3, 3), 6.0, dtype or np.float64)) if positions == "given" else None
        if not moved:
            return gpu.prev_points_host(hits, pos, device=3)
        sp, sc = _spheres(spheres, lambda k: np.full((k, 4), 7.0, dtype or np.float64))
        names.add("spheres_prev", sp), names.add("spheres_cur", sc)
        return gpu.prev_points_moved_host(hits, pos, sp, sc, device=3)
    return run


for _n, _p in itertools.product((3, 0), ("none", "given")):
    for _o in ("none", "given", "point"):
        T[f"prev_points-n{_n}-positions_{_p}-out_{_o}"] = _prev_points(False, _n, _p, None, _o)
        for _s in ("none", "empty", "given"):
            T[f"prev_points_moved-n{_n}-positions_{_p}-spheres_{_s}-out_{_o}"] = _prev_points(True, _n, _p, _s, _o)
    T[f"prev_points_host-n{_n}-positions_{_p}"] = _prev_points_host(False, _n, _p, None)
    for _s in ("none", "empty", "given"):
        T[f"prev_points_moved_host-n{_n}-positions_{_p}-spheres_{_s}"] = _prev_points_host(True, _n, _p, _s)
T["prev_points-positions_strided"] = _prev_points(False, 3, "strided", None, "none")
T["prev_points_moved-positions_strided"] = _prev_points(True, 3, "strided", "given", "none")
T["prev_points_host-converted"] = _prev_points_host(False, 3, "given", None, np.float32)
T["prev_points_moved_host-converted"] = _prev_points_host(True, 3, "given", "given", np.float32)


def _out_dict(names, kind, fields, optional):
    """the `out` of reproject / upsample: missing, partly given, the optional fields None, everything given"""
    if kind == "missing":
        return None
    out = names.add("out", {f: z(*shape, dtype=dtype) for f, (shape, dtype) in fields.items()})
    if kind == "partly":
        return {f: out[f] for f in list(fields)[:1]}
    if kind == "optional_none":
        return {f: (None if f in optional else out[f]) for f in fields}
    if kind == "one_none":
        return {optional[0]: None}
    return out


REPROJECT_OUT = dict(rgb=((H, W, 3), F32), len=((H, W), F32), motion=((H, W, 2), F32), rgb8=((H, W, 3), U8))
UPSAMPLE_OUT = dict(rgb=((H, W, 3), F32), rgb8=((H, W, 3), U8), conf=((H, W), F32))
OUT_KINDS = ("missing", "partly", "optional_none", "one_none", "given")


def _reproject(hist, points, out):
    def run(rec, names):
        rgb, aov, cam = names.add("rgb", z(H, W, 3)), names.add("aov", aov_t(W, H)), names.add("camera", abi.Camera())
        h = names.add("hist", dict(rgb=z(H, W, 3), len=z(H, W), aov=aov_t(W, H), camera=abi.Camera())) if hist else None
        p = names.add("prev_points", z(H, W, 3, dtype=F64)) if points else None
        o = _out_dict(names, out, REPROJECT_OUT, ("motion", "rgb8"))
        if out == "partly":
            o = dict(o, rgb=rgb)   # (it may be the input rgb)
        return gpu.reproject(rgb, aov, cam, hist=h, out=o, prev_points=p, max_history=8.0)
    return run


def _reproject_host(hist, points, dtype=None):
    def run(rec, names):
        rgb, aov, cam = names.add("rgb", np.full((H, W, 3), 9.0, dtype or np.float32)), names.add("aov", aov_np(W, H, dtype)), abi.Camera()
        names.add("camera", cam)
        h = None
        if hist:
            h = names.add("hist", dict(rgb=np.full((H, W, 3), 10.0, dtype or np.float32), len=np.full((H, W), 11.0, dtype or np.float32),
                                       aov=aov_np(W, H, dtype), camera=abi.Camera()))
        p = names.add("prev_points", np.full((H, W, 3), 12.0, np.float32 if dtype else np.float64)) if points else None
        return gpu.reproject_image_host(rgb, aov, cam, hist=h, device=3, prev_points=p, depth_tol=0.5)
    return run


for _h, _p in itertools.product((False, True), (False, True)):
    for _o in OUT_KINDS:
        T[f"reproject-hist_{_h}-points_{_p}-out_{_o}"] = _reproject(_h, _p, _o)
    T[f"reproject_image_host-hist_{_h}-points_{_p}"] = _reproject_host(_h, _p)
T["reproject_image_host-converted"] = _reproject_host(True, True, np.float64)


def _upsample(flags, out):
    def run(rec, names):
        low_rgb, low_aov, aov = names.add("low_rgb", z(HL, WL, 3)), names.add("low_aov", aov_t(WL, HL)), names.add("aov", aov_t(W, H))
        kw = dict(demodulate=True, object_edges=True) if flags else dict(sigma_depth=0.25)
        if not flags:   # what the flags do not ask for may be missing
            low_aov, aov = ({f: a[f] for f in ("normal", "depth", "hits")} for a in (low_aov, aov))
        return gpu.upsample(low_rgb, low_aov, WL, HL, aov, W, H, out=_out_dict(names, out, UPSAMPLE_OUT, ("rgb8", "conf")), **kw)
    return run


def _upsample_host(kind):
    def run(rec, names):
        dtype = np.float64 if kind == "converted" else None
        low_rgb = names.add("low_rgb", np.full((HL, WL, 3), 9.0, dtype or np.float32))
        low_aov, aov = names.add("low_aov", aov_np(WL, HL, dtype)), names.add("aov", aov_np(W, H, dtype))
        if kind == "partly":   # a field missing, a field None
            low_aov = {f: v for f, v in low_aov.items() if f != "object"}
            aov = dict(aov, albedo=None)
        kw = dict(demodulate=True, object_edges=True) if kind == "flags" else {}
        return gpu.upsample_image_host(low_rgb, low_aov, aov, device=3, **kw)
    return run


for _f in (False, True):
    for _o in OUT_KINDS:
        T[f"upsample-flags_{_f}-out_{_o}"] = _upsample(_f, _o)
for _k in ("plain", "flags", "partly", "converted"):
    T[f"upsample_image_host-{_k}"] = _upsample_host(_k)


def _render_tiles(kind):
    def run(rec, names):
        gs = scene_stub(rec, names)
        kw = dict(tiles=names.add("tiles", z(2, 64, 3)), tiles8=names.add("tiles8", z(2, 64, 3, dtype=U8)), stats=names.add("stats", z(4, dtype=I64)))
        if kind == "allocated":
            kw = {}
        if kind == "chunks":
            kw["chunks"] = 2
        if kind == "workspace":
            kw.update(chunks=2, workspace=names.add("workspace", z(64, dtype=U8)), camera=names.add("camera", abi.Camera()), samples=2, max_depth=3)
        return gpu.GpuScene.render_tiles(gs, 7, 0, 1, 2, **kw)
    return run


for _k in ("given", "allocated", "chunks", "workspace"):
    T[f"render_tiles-{_k}"] = _render_tiles(_k)


def _untile(kind):
    def run(rec, names):
        gs = scene_stub(rec, names)
        tiles, tiles8 = names.add("tiles", z(2, 64, 3)), names.add("tiles8", z(2, 64, 3, dtype=U8))
        if kind == "no_bytes":
            return gs.untile(tiles, None, 0, 1, 2)
        if kind == "into":
            return gs.untile(tiles, tiles8, 1, 2, 1, image=names.add("image", z(H, W, 3)), image8=names.add("image8", z(H, W, 3, dtype=U8)))
        if kind == "into_no_bytes":
            return gs.untile(tiles, None, 0, 1, 2, image=names.add("image", z(H, W, 3)))
        return gs.untile(tiles, tiles8, 0, 1, 2)
    return run


for _k in ("plain", "no_bytes", "into", "into_no_bytes"):
    T[f"untile-{_k}"] = _untile(_k)


def _render_aov(kind):
    def run(rec, names):
        gs = scene_stub(rec, names)
        if kind == "subset":
            return gs.render_aov(7, 2, first=1, stride=2, count=1, camera=names.add("camera", abi.Camera()), want=("normal", "hits"))
        if kind == "empty":
            return gs.render_aov(7, 2, count=0)
        return gs.render_aov(7, 2)
    return run


for _k in ("plain", "subset", "empty"):
    T[f"render_aov-{_k}"] = _render_aov(_k)


def _untile_aov(kind):
    def run(rec, names):
        gs = scene_stub(rec, names)
        tiles = dict(albedo=z(2, 64, 3), normal=z(2, 64, 3), depth=z(2, 64), object=z(2, 64, dtype=I32), hits=z(2, 64, dtype=I32))
        if kind == "subset":
            tiles = {f: tiles[f] for f in ("hits", "depth")}
        return gs.untile_aov(names.add("tiles", tiles), 0, 1, 2)
    return run


for _k in ("plain", "subset"):
    T[f"untile_aov-{_k}"] = _untile_aov(_k)


def _accumulation(kind):
    def run(rec, names):
        gs = scene_stub(rec, names)
        acc = gpu.Accumulation(gs, names.add("accum", C.c_void_p(0xACC00000)), 2, seed=7)
        if kind == "resolve":
            out = acc.resolve()
        elif kind == "resolve_into":
            out = acc.resolve(tiles=names.add("tiles", z(2, 64, 3)), tiles8=names.add("tiles8", z(2, 64, 3, dtype=U8)))
        elif kind == "add":
            out = (acc.add(2), acc.add(3, stats=names.add("stats", z(4, dtype=I64))))
        acc.handle = None
        return out
    return run


for _k in ("resolve", "resolve_into", "add"):
    T[f"accumulation-{_k}"] = _accumulation(_k)


def _aov_image_host(rec, names):
    sc = types.SimpleNamespace(width=W, height=H, objects=None, n_objects=0, n_meshes=0, hip_meshes=lambda: None,
                               camera=names.add("scene.camera", abi.Camera()))
    return gpu.aov_image_host(sc, 7, 2, device=3)


T["aov_image_host"] = _aov_image_host


def _temporal(rec, names):
    """two frames of a Temporal: without a history, then with one and the spheres of the frame before"""
    gs = scene_stub(rec, names)
    t = gpu.Temporal(gs, max_history=8.0)
    names.add("slot", t._slots), names.add("tiles", t._tiles), names.add("tiles8", t._tiles8), names.add("motion", t._motion)
    names.add("rgb8", t._rgb8), names.add("uv", t._uv), names.add("hits", t._hits), names.add("points", t._points)
    gs._spheres = names.add("spheres", z(2, 4, dtype=F64))
    cam = names.add("camera", abi.Camera())
    first = t.frame(cam, 7, 2)
    first = names.describe(names.add("first", first))
    return dict(first=first, second=t.frame(cam, 8, 2, prev_spheres=names.add("prev_spheres", z(2, 4, dtype=F64))))


T["temporal-two_frames"] = _temporal


# ---- (b) the refusals --------------------------------------------------------------------------------------------------------------------------------
R = {}


def _with(base, **broken):
    """the valid arguments of `base` with some replaced: a callable gets the valid value"""
    args = base()
    for k, v in broken.items():
        path = k.split("__")
        d = args
        for q in path[:-1]:
            d[q] = dict(d[q])
            d = d[q]
        d[path[-1]] = v(d.get(path[-1])) if callable(v) else v
    return args


def double(t):
    return t.double()


def longs(t):
    return t.long()


def short(t):
    return t.reshape(-1)[1:].clone()


def drop(_):
    return _DROP


_DROP = object()


def _strip(d):
    return {k: (_strip(v) if isinstance(v, dict) else v) for k, v in d.items() if v is not _DROP}


def _refusals(name, base, call, cases):
    for tag, broken in cases.items():
        R[f"{name}-{tag}"] = (lambda broken=broken: call(**_strip(_with(base, **broken))))


_refusals("tile_error", lambda: dict(cur=z(2, 64, 3), prev=z(2, 64, 3), out=None),
          lambda cur, prev, out: gpu.tile_error(cur, prev, W, H, out=out),
          dict(cur_dtype=dict(cur=double), prev_dtype=dict(prev=double), prev_device=dict(prev=meta), cur_strided=dict(cur=strided),
               prev_count=dict(prev=short)))

_refusals("denoise", lambda: dict(rgb=z(H, W, 3), aov=aov_t(W, H), out=None),
          lambda rgb, aov, out: gpu.denoise(rgb, aov, W, H, out=out),
          dict(rgb_strided=dict(rgb=strided), depth_strided=dict(aov__depth=strided), hits_device=dict(aov__hits=meta),
               stranger_strided=dict(aov__variance=lambda _: strided(z(H, W))),
               rgb_dtype=dict(rgb=double), rgb_count=dict(rgb=short), depth_count=dict(aov__depth=short), albedo_count=dict(aov__albedo=short),
               out_dtype=dict(out=lambda _: z(H, W, 3, dtype=F64)), out_count=dict(out=lambda _: z(H, W)),
               out_strided=dict(out=lambda _: strided(z(H, W, 3))), out_device=dict(out=lambda _: meta(z(H, W, 3))),
               first_strided_then_dtype=dict(rgb=double, aov__depth=strided), first_rgb_then_count=dict(rgb=double, aov__depth=short),
               first_count_then_out=dict(aov__normal=short, out=lambda _: z(H, W)),
               first_albedo_then_hits=dict(aov__albedo=short, aov__hits=short)))

_refusals("select_pixels", lambda: dict(values=z(H, W), capacity=None, indices=None),
          lambda values, capacity, indices: gpu.select_pixels(values, W, H, 0.0, 1.0, capacity=capacity, indices=indices),
          dict(values_dtype=dict(values=double), values_strided=dict(values=strided), values_count=dict(values=short),
               indices_dtype=dict(indices=z(45, dtype=I64)), indices_strided=dict(indices=strided(z(45, dtype=I32))),
               indices_device=dict(indices=meta(z(45, dtype=I32))), indices_short=dict(capacity=4, indices=z(3, dtype=I32)),
               first_values_then_indices=dict(values=double, indices=z(45, dtype=I64))))

_refusals("blend_pixels", lambda: dict(pixels=z(3, dtype=I32), status=z(3, dtype=I32), radiance=z(3, 3, dtype=F64), rgb=z(H, W, 3), prior=None,
                                       rgb8=None, weight=None, n=None),
          lambda pixels, status, radiance, rgb, **kw: gpu.blend_pixels(pixels, status, radiance, rgb, W, H, 4.0, 0.5, **kw),
          dict(pixels_float=dict(pixels=z(3)), pixels_long=dict(pixels=z(3, dtype=I64)),
               n_negative=dict(n=-1), n_beyond=dict(n=4), status_short=dict(status=short), radiance_short=dict(radiance=lambda t: t[:2].clone()),
               status_long=dict(status=longs), status_strided=dict(status=strided), status_device=dict(status=meta),
               radiance_dtype=dict(radiance=lambda t: t.float()), radiance_strided=dict(radiance=strided), radiance_device=dict(radiance=meta),
               rgb_dtype=dict(rgb=double), rgb_strided=dict(rgb=strided), rgb_count=dict(rgb=short),
               prior_dtype=dict(prior=z(H, W, dtype=F64)), prior_count=dict(prior=z(H, W, 3)), prior_device=dict(prior=meta(z(H, W))),
               weight_dtype=dict(weight=z(H, W, dtype=F64)), weight_strided=dict(weight=strided(z(H, W))),
               rgb8_dtype=dict(rgb8=z(H, W, 3)), rgb8_count=dict(rgb8=z(H, W, dtype=U8)),
               first_pixels_then_n=dict(pixels=z(3), n=-1), first_n_then_status=dict(n=4, status=longs),
               first_status_then_rgb=dict(radiance=strided, rgb=double), first_rgb_then_prior=dict(rgb=short, prior=z(H, W, 3)),
               first_prior_then_weight=dict(prior=z(H, W, 3), weight=z(H, W, 3)), first_weight_then_rgb8=dict(weight=z(H, W, 3), rgb8=z(H, W, 3))))

_HIT_BREAKS = dict(dtype=lambda t: t.float() if t.is_floating_point() else t.long(), strided=strided, device=meta,
                   count=lambda t: torch.cat([t, t]))


def _points_cases(moved):
    fields = ("status", "prim", "object", "bary", "point") if moved else ("status", "prim", "bary", "point")
    cases = {f"hits_{f}_{how}": {f"hits__{f}": fn} for f in fields[1:] for how, fn in _HIT_BREAKS.items()}
    cases.update(hits_status_dtype={"hits__status": longs}, hits_status_strided={"hits__status": strided},
                 hits_status_count={"hits__status": short},      # (status sets n: the refusal names the next field's count)
                 hits_status_device={"hits__status": meta},
                 positions_dtype=dict(positions=lambda t: t.float()), positions_dim=dict(positions=lambda t: t.reshape(2, 9)),
                 positions_shape=dict(positions=lambda t: z(2, 3, 4, dtype=F64)), positions_device=dict(positions=meta),
                 out_dtype=dict(out=z(3, 3)), out_count=dict(out=z(4, 3, dtype=F64)), out_strided=dict(out=strided(z(3, 3, dtype=F64))),
                 out_device=dict(out=meta(z(3, 3, dtype=F64))),
                 first_prim_then_point={"hits__prim": longs, "hits__point": strided},
                 first_hits_then_positions={"hits__point": strided, "positions": lambda t: t.float()},
                 first_positions_then_out=dict(positions=lambda t: t.float(), out=z(3, 3)))
    if moved:
        cases.update(spheres_prev_alone=dict(spheres_cur=None), spheres_cur_alone=dict(spheres_prev=None),
                     spheres_dtype=dict(spheres_prev=lambda t: t.float()), spheres_dim=dict(spheres_cur=lambda t: t.reshape(-1)),
                     spheres_width=dict(spheres_cur=z(2, 3, dtype=F64)), spheres_device=dict(spheres_prev=meta),
                     spheres_shapes=dict(spheres_cur=z(3, 4, dtype=F64)),
                     first_positions_then_spheres=dict(positions=lambda t: t.float(), spheres_cur=None),
                     first_alone_then_dtype=dict(spheres_prev=None, spheres_cur=lambda t: t.float()),
                     first_prev_then_cur=dict(spheres_prev=lambda t: t.float(), spheres_cur=z(3, 4, dtype=F64)),
                     first_spheres_then_out=dict(spheres_cur=z(3, 4, dtype=F64), out=z(3, 3)))
    return cases


_refusals("prev_points", lambda: dict(hits=hits_t(3, False), positions=z(2, 3, 3, dtype=F64), out=None),
          lambda hits, positions, out: gpu.prev_points(hits, positions, out=out), _points_cases(False))
_refusals("prev_points_moved", lambda: dict(hits=hits_t(3), positions=z(2, 3, 3, dtype=F64), spheres_prev=z(2, 4, dtype=F64),
                                            spheres_cur=z(2, 4, dtype=F64), out=None),
          lambda hits, positions, spheres_prev, spheres_cur, out: gpu.prev_points_moved(hits, positions, spheres_prev, spheres_cur, out=out),
          _points_cases(True))


def _np_twice(a):
    return np.concatenate([a, a])


_refusals("prev_points_host", lambda: dict(hits=hits_np(3, False), positions=np.zeros((2, 3, 3))),
          lambda hits, positions: gpu.prev_points_host(hits, positions),
          dict(prim_count={"hits__prim": _np_twice}, bary_count={"hits__bary": _np_twice}, point_count={"hits__point": _np_twice},
               status_count={"hits__status": _np_twice}, first_prim_then_point={"hits__prim": _np_twice, "hits__point": _np_twice}))
_refusals("prev_points_moved_host", lambda: dict(hits=hits_np(3), positions=np.zeros((2, 3, 3)), spheres_prev=np.zeros((2, 4)),
                                                 spheres_cur=np.zeros((2, 4))),
          lambda **kw: gpu.prev_points_moved_host(**kw),
          dict(prim_count={"hits__prim": _np_twice}, object_count={"hits__object": _np_twice}, bary_count={"hits__bary": _np_twice},
               point_count={"hits__point": _np_twice}, status_count={"hits__status": _np_twice},
               spheres_prev_alone=dict(spheres_cur=None), spheres_cur_alone=dict(spheres_prev=None), spheres_shapes=dict(spheres_cur=np.zeros((3, 4))),
               first_hits_then_spheres={"hits__object": _np_twice, "spheres_cur": None}))


def _aov_cases(key, fields):
    cases = {}
    for f in fields:
        cases.update({f"{key}_{f}_strided": {f"{key}__{f}": strided}, f"{key}_{f}_device": {f"{key}__{f}": meta},
                      f"{key}_{f}_count": {f"{key}__{f}": short}})
    cases.update({f"{key}_depth_wide": {f"{key}__depth": double}, f"{key}_hits_wide": {f"{key}__hits": longs},
                  f"{key}_hits_narrow": {f"{key}__hits": lambda t: t.to(torch.int16)}})
    return cases


def _out_cases(fields):
    cases = {}
    for f, (shape, dtype) in fields.items():
        cases.update({f"out_{f}_dtype": {f"out__{f}": z(*shape, dtype=F64)}, f"out_{f}_strided": {f"out__{f}": strided(z(*shape, dtype=dtype))},
                      f"out_{f}_device": {f"out__{f}": meta(z(*shape, dtype=dtype))}, f"out_{f}_count": {f"out__{f}": z(2, dtype=dtype)}})
    return cases


_refusals("reproject", lambda: dict(rgb=z(H, W, 3), aov=aov_t(W, H), hist=dict(rgb=z(H, W, 3), len=z(H, W), aov=aov_t(W, H), camera=abi.Camera()),
                                    out={}, prev_points=z(H, W, 3, dtype=F64)),
          lambda rgb, aov, hist, out, prev_points: gpu.reproject(rgb, aov, abi.Camera(), hist=hist, out=out, prev_points=prev_points),
          dict(rgb_dim=dict(rgb=lambda t: t.reshape(-1)), rgb_channels=dict(rgb=z(H, W, 4)), rgb_dtype=dict(rgb=double), rgb_strided=dict(rgb=strided),
               **_aov_cases("aov", gpu.REPROJECT_AOV), **_aov_cases("hist__aov", gpu.REPROJECT_AOV),
               hist_rgb_dtype=dict(hist__rgb=double), hist_rgb_strided=dict(hist__rgb=strided), hist_rgb_device=dict(hist__rgb=meta),
               hist_rgb_count=dict(hist__rgb=short), hist_len_dtype=dict(hist__len=double), hist_len_count=dict(hist__len=short),
               **_out_cases(REPROJECT_OUT),
               points_dtype=dict(prev_points=lambda t: t.float()), points_strided=dict(prev_points=strided), points_device=dict(prev_points=meta),
               points_count=dict(prev_points=short),
               first_rgb_then_aov=dict(rgb=double, aov__depth=short), first_normal_then_hits=dict(aov__normal=short, aov__hits=short),
               first_frame_then_history=dict(aov__hits=short, hist__rgb=double), first_history_rgb_then_len=dict(hist__rgb=short, hist__len=short),
               first_history_len_then_aov=dict(hist__len=short, hist__aov__normal=short),
               first_history_then_out=dict(hist__aov__hits=short, out__rgb=z(2)), first_out_rgb_then_rgb8=dict(out__rgb=z(2), out__rgb8=z(2, dtype=U8)),
               first_out_then_points=dict(out__rgb8=z(2, dtype=U8), prev_points=short)))

_refusals("reproject_image_host", lambda: dict(prev_points=np.zeros((H, W, 3))),
          lambda prev_points: gpu.reproject_image_host(np.zeros((H, W, 3), np.float32), aov_np(W, H), abi.Camera(), prev_points=prev_points),
          dict(points_count=dict(prev_points=np.zeros((H, W, 2)))))

_UP_FIELDS = ("normal", "depth", "hits", "albedo", "object")
_refusals("upsample", lambda: dict(low_rgb=z(HL, WL, 3), low_aov=aov_t(WL, HL), aov=aov_t(W, H), out={}, flags=dict(demodulate=True, object_edges=True)),
          lambda low_rgb, low_aov, aov, out, flags: gpu.upsample(low_rgb, low_aov, WL, HL, aov, W, H, out=out, **flags),
          dict(low_rgb_dtype=dict(low_rgb=double), low_rgb_strided=dict(low_rgb=strided), low_rgb_count=dict(low_rgb=short),
               **{f"low_{f}_missing": {f"low_aov__{f}": drop} for f in _UP_FIELDS}, **{f"full_{f}_missing": {f"aov__{f}": drop} for f in _UP_FIELDS},
               **_aov_cases("low_aov", _UP_FIELDS), **_aov_cases("aov", _UP_FIELDS), **_out_cases(UPSAMPLE_OUT),
               first_low_rgb_then_missing={"low_rgb": double, "low_aov__normal": drop},
               first_missing_normal_then_bad_depth={"low_aov__normal": drop, "low_aov__depth": short},
               first_bad_normal_then_missing_depth={"low_aov__normal": short, "low_aov__depth": drop},
               first_hits_then_albedo={"aov__hits": short, "aov__albedo": drop},
               first_albedo_then_object={"aov__albedo": short, "aov__object": drop},
               first_low_then_full={"low_aov__object": short, "aov__normal": drop},
               first_full_then_out={"aov__object": short, "out__rgb": z(2)},
               first_out_rgb_then_conf={"out__rgb": z(2), "out__conf": z(2)}))


def _refusal(mp, fn):
    _patch(mp, Recorder())
    with pytest.raises(ValueError) as e:
        fn()
    return str(e.value)


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
    got = _transcript(monkeypatch, T[case])
    assert got["calls"], case
    assert got == _golden()["transcripts"][case]


@pytest.mark.parametrize("case", sorted(R))
def test_refusal(monkeypatch, case):
    assert _refusal(monkeypatch, R[case]) == _golden()["refusals"][case]


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: test_image_front_calls.py --record"
    recorded = dict(transcripts={}, refusals={})
    for case in sorted(T):
        with pytest.MonkeyPatch.context() as mp:
            recorded["transcripts"][case] = _transcript(mp, T[case])
    for case in sorted(R):
        with pytest.MonkeyPatch.context() as mp:
            recorded["refusals"][case] = _refusal(mp, R[case])
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(T)} transcripts, {len(R)} refusals -> {GOLDEN}")
