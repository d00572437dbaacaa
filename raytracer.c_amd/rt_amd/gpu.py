"""Python driver of the HIP shim (include/rt_hip.h).  PyTorch is used for what it is
good at here -- device buffers, streams, torch.distributed -- and nothing else: every
pixel is computed by librt_hip.so.  There is no CPU / eager fallback: if the shim is
missing or no GPU is visible, calls raise.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import abi
from .dist import n_tiles, rank_tiles  # noqa: F401  (re-exported)


class ShimError(RuntimeError):
    pass


def _check(rc, what):
    if rc != 0:
        msg = abi.load_shim().rt_hip_last_error()
        raise ShimError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def _stats_dict(stats):
    """the four counters of a call (RT_HIP_NSTATS words, abi.STAT_* order) by name"""
    return dict(rays=stats[0], casts=stats[1], tests=stats[2], samples=stats[3])


def _distance(xyz):
    """|xyz|: how far a camera or a ray origin is from the world's origin, the default origin_radius of its rays"""
    x, y, z = xyz
    return (x * x + y * y + z * z) ** 0.5


def _device_rays(rays, per_ray, dev):
    """rays or uv pairs as a contiguous float64 tensor [n, per_ray] on `dev` that starts on a 16-byte boundary"""
    rays = torch.as_tensor(rays, dtype=torch.float64, device=dev).reshape(-1, per_ray).contiguous()
    return rays.clone() if rays.data_ptr() % 16 else rays   # (a view into a larger tensor: the kernel loads 16 bytes at a time)


_TORCH = {"float32": torch.float32, "float64": torch.float64, "uint32": torch.int32, "uint64": torch.int64}   # (the C-ABI's words, as torch holds them)


def _stream(dev):
    """torch's current stream on `dev`, as the shim takes it"""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    """a tensor's address as the shim takes it (None: a null pointer)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _some(t, some=True):
    """... of a tensor that may be missing or empty, or of which nothing is to be read (some false): a null c_void_p then"""
    return C.c_void_p(t.data_ptr() if t is not None and some and t.numel() else None)


def _camera(scene, camera):
    """the camera of a call: the one given, or the scene's own"""
    return camera if camera is not None else scene.camera


def _depth(scene, max_depth):
    """the max_depth of a call: the one given (0 is one), or the scene's own"""
    return scene.max_depth if max_depth is None else max_depth


def _params(scene, seed, samples, max_depth, integrator="path", tiles=(0, 0, 0)):
    """the one RtHipParams builder: the scene's size, and (first, stride, count) of the tiles where a call has them"""
    p = abi.RtHipParams()
    p.integrator = abi.INTEGRATORS[integrator]
    p.width, p.height, p.samples, p.max_depth, p.seed = scene.width, scene.height, samples, max_depth, seed
    p.tile_first, p.tile_stride, p.tile_count = tiles
    return p


def _counters(dev, stats=None):
    """the counters of a device call (int64 [RT_HIP_NSTATS]): the tensor given, which the call adds to, or zeros"""
    return torch.zeros(abi.NSTATS, dtype=torch.int64, device=dev) if stats is None else stats


def _host_counters():
    """... of a host form"""
    return (C.c_uint64 * abi.NSTATS)()


def _host_scene(scene):
    """the four leading arguments of a scene-owning host form (hip_meshes()' result lives in the call's arguments)"""
    return scene.objects, scene.n_objects, scene.hip_meshes(), scene.n_meshes


def _points3(x, dev, dtype=torch.float64):
    """positions, normals or colours as a contiguous [N, 3] tensor on `dev`"""
    return torch.as_tensor(x, dtype=dtype, device=dev).reshape(-1, 3).contiguous()


def _frame_pair(h, w, dev):
    """(rgb float32 [h, w, 3], rgb8 uint8 [h, w, 3]) for a call to fill: on `dev`, or numpy arrays with dev None"""
    if dev is None:
        return np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w, 3), dtype=np.uint8)
    return torch.empty((h, w, 3), dtype=torch.float32, device=dev), torch.empty((h, w, 3), dtype=torch.uint8, device=dev)


def _workspace(nbytes, dev):
    """a byte workspace of a generated-ray job: at least 256 bytes"""
    return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)


def _grid_count(grid):
    return grid.count[0] * grid.count[1] * grid.count[2]


def _grid_radius(grid):
    """the default origin_radius of a grid's probes: its farthest corner from the world's origin, a shade more"""
    far = [max(abs(grid.origin[a]), abs(grid.origin[a] + (grid.count[a] - 1) * grid.step[a])) for a in range(3)]
    return _distance(far) * (1.0 + 2.0 ** -40)


def _moments(moments, grid, vis, dev, who):
    """a grid's depth moments as a contiguous float64 tensor on `dev`: R*R x 2 values a probe"""
    t = torch.as_tensor(moments, dtype=torch.float64, device=dev).contiguous()
    if t.numel() != _grid_count(grid) * vis.res * vis.res * 2:
        raise ValueError(f"{who}: moments must hold {vis.res} x {vis.res} x 2 values per probe of the grid")
    return t


def _slices(n, samples, slice_rays):
    """(slice_rays, rays a launch) of a sliced bake of n probes: None is everything at once, and a launch has 1 .. total rays"""
    total = max(n * samples, 1)
    slice_rays = total if slice_rays is None else slice_rays
    return slice_rays, max(min(slice_rays, total), 1)


def _is(t, dev=None, n=None, dtype=None, size=None):
    """The one tensor requirement: t is contiguous and -- of what is asked -- on `dev`, of n values, of this dtype, of this element
    size.  The caller says what it asks and keeps its own refusal."""
    return (dev is None or t.device == dev) and t.is_contiguous() and (n is None or t.numel() == n) and \
        (dtype is None or t.dtype == dtype) and (size is None or t.element_size() == size)


def _wanted(record, shapes, want, n, dev, samples=0, into=None):
    """The outputs `want` of an RtHipHits or an RtHipRadiance (`record`; shapes: abi.HIT_SHAPES or abi.RADIANCE_SHAPES) for n entries
    -> (dict, record): tensors on `dev` (the C-ABI's uint32 / uint64 words as int32 / int64; a field of `into` is used where given), or
    numpy arrays with dev None.  Each one's address goes into the record's field (n == 0 launches nothing: it only says "wanted")."""
    out = {}
    for f in want:
        dtype, k = shapes[f]
        shape = (n, samples, 3) if f == "samples" else ((n, k) if k > 1 else (n,))
        if into is not None and f in into:
            out[f] = t = into[f]
            if not _is(t, dev, dtype=_TORCH[dtype]) or tuple(t.shape) != shape:
                raise ValueError(f"query: out[{f!r}] must be a contiguous {_TORCH[dtype]} tensor of shape {shape} on the scene's device")
        else:
            out[f] = np.zeros(shape, dtype=dtype) if dev is None else torch.empty(shape, dtype=_TORCH[dtype], device=dev)
        setattr(record, f, (out[f].ctypes.data if dev is None else out[f].data_ptr()) if n else 1)
    return out, record


def _aov_record(bufs, fields, check=None, optional=False, host=False):
    """The one RtHipAov builder: the addresses of bufs[f] for f in `fields`, device tensors or -- host -- arrays, which are converted to
    the field's type (abi.AOV_DTYPES) and stay alive with the record.  optional: a field that is missing or None stays null.
    check(f, buffer): the caller's requirement of a field; it raises the caller's refusal."""
    a = abi.RtHipAov()
    a.kept = []
    for f in fields:
        t = bufs.get(f) if optional else bufs[f]
        if check is not None:
            check(f, t)
        if t is None:
            continue
        if host:
            t = np.ascontiguousarray(t, dtype=abi.AOV_DTYPES[f])
            a.kept.append(t)
        setattr(a, f, t.ctypes.data if host else t.data_ptr())
    return a


def _aov_shape(f, *lead):
    """the shape of field f's buffer of lead pixels: a trailing 3 where the field has three channels"""
    return lead + ((3,) if abi.AOV_CHANNELS[f] == 3 else ())


class GpuScene:
    """A scene resident in HBM (rt_hip_scene_create_opts).  bvh: who builds the triangle hierarchy, "host" (the default) or
    "device" -- frames, bytes and counters are the same under either."""

    def __init__(self, scene, device=0, bvh="host"):
        if bvh not in abi.BVH_BUILDERS:
            raise ValueError(f"bvh must be one of {sorted(abi.BVH_BUILDERS)}, not {bvh!r}")
        self.shim = abi.load_shim()
        if self.shim.rt_hip_device_count() < 1:
            raise ShimError("no HIP device visible; this package has no CPU fallback")
        self.scene = scene
        self.device = device
        handle = C.c_void_p()
        opts = abi.RtHipSceneOptions()
        self.shim.rt_hip_scene_options_defaults(C.byref(opts))
        opts.bvh_builder = abi.BVH_BUILDERS[bvh]
        objects, n_objects, self._meshes, n_meshes = _host_scene(scene)
        _check(self.shim.rt_hip_scene_create_opts(objects, n_objects, self._meshes, n_meshes, device, C.byref(opts), C.byref(handle)),
               "rt_hip_scene_create_opts")
        self.handle = handle
        self._accums = []  # handles of the accumulations made here: closed before the scene (rt_hip.h: the scene outlives them)

    @property
    def dev(self):
        """the scene's device, as torch names it"""
        return torch.device("cuda", self.device)

    def close(self):
        if self.handle:
            # first whatever accumulation is still open: the garbage collector finalises a scene and its accumulations in any
            # order when they die together, and rt_hip_accum_destroy reads the scene
            for h in self._accums:
                if h:
                    self.shim.rt_hip_accum_destroy(h)
                    h.value = None
            self._accums = []
            self.shim.rt_hip_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def params(self, seed, first, stride, count, samples=None, max_depth=None, integrator="path"):
        return _params(self.scene, seed, samples or self.scene.samples, _depth(self.scene, max_depth), integrator, (first, stride, count))

    def kernel_name(self, integrator="path"):
        return self.shim.rt_hip_kernel_name(self.handle, abi.INTEGRATORS[integrator]).decode()

    def last_launch_kernel(self):
        """the kernel this thread's last render_tiles() launched (the launch's own facts can name another than kernel_name())"""
        return self.shim.rt_hip_last_launch_kernel().decode()

    def launch_status(self):
        """device-side failures of render launches since the last call (0 = none); raises ShimError when any"""
        flags = C.c_uint32(0)
        _check(self.shim.rt_hip_launch_status(self.device, C.byref(flags)), "rt_hip_launch_status")
        return flags.value

    def hull_facets(self):
        """(triangles marked as hull facets with the stored normal pointing outward, ... inward)"""
        plus, minus = C.c_uint32(0), C.c_uint32(0)
        _check(self.shim.rt_hip_scene_hull_facets(self.handle, C.byref(plus), C.byref(minus)), "rt_hip_scene_hull_facets")
        return plus.value, minus.value

    def bvh_info(self):
        """the triangle hierarchy: builder ("host" / "device"), depth, max_depth, n_nodes, tree_cost (the expected instructions
        of a walk per ray that meets the root's box) and build_seconds"""
        b, d, md, nn, cost = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_double(0)
        _check(self.shim.rt_hip_scene_bvh_info(self.handle, C.byref(b), C.byref(d), C.byref(md), C.byref(nn), C.byref(cost)),
               "rt_hip_scene_bvh_info")
        names = {v: k for k, v in abi.BVH_BUILDERS.items()}
        return {"builder": names[b.value], "depth": d.value, "max_depth": md.value, "n_nodes": nn.value, "tree_cost": cost.value,
                "build_seconds": float(self.shim.rt_hip_scene_bvh_build_seconds(self.handle))}

    def bvh_read(self):
        """(nodes, order): the fp64 source nodes as an (n_nodes, 16) float64 array -- two child boxes, the two refs in the
        bytes of column 12 -- and the leaf order as uint32 triangle indices"""
        info = self.bvh_info()
        nodes = np.zeros((info["n_nodes"], abi.BVH_SRC_DOUBLES), dtype=np.float64)
        order = np.zeros(self.scene.n_triangles, dtype=np.uint32)
        _check(self.shim.rt_hip_scene_bvh_read(self.handle, nodes.ctypes.data if nodes.size else None,
                                               order.ctypes.data if order.size else None), "rt_hip_scene_bvh_read")
        return nodes, order

    def update_vertices(self, positions, rebuild_above=None):
        """Moves the scene's triangles in place (rt_hip.h, rt_hip_scene_update_vertices): positions of shape (n, 3, 3) -- triangle,
        corner, xyz, in scene triangle order -- as a float64 torch tensor on the scene's device (taken where it lies, no host
        copy) or a numpy array (staged by the shim).  Synchronous.  The records are recomputed and the hierarchy REFITTED on the
        device: frames, bytes and counters equal a freshly created scene's.  rebuild_above: None leaves the refitted tree as it
        is; a ratio >= 1 ends the update with maintain_bvh(rebuild_above), whose result is returned (None otherwise): the tree
        is rebuilt in place when the refit has made it that much dearer than it was built.  A Temporal keeps its history
        across an update when its next frame() is given the positions from before it (prev_positions); without them, and for a
        Preview, which assumes a static scene, reset after an update.  Open accumulations refuse the update (close them first).
        self.scene keeps the vertices the scene was created from."""
        self._update("update_vertices", positions, (self.scene.n_triangles, 3, 3))
        return None if rebuild_above is None else self.maintain_bvh(rebuild_above)

    def _update(self, name, x, shape):
        """The one body of update_vertices / update_spheres (rt_hip_scene_<name>, or its _host form for what is no tensor) -> what
        went down: the contiguous tensor, or the float64 array"""
        symbol = "rt_hip_scene_" + name
        if isinstance(x, torch.Tensor):
            if x.dtype != torch.float64 or tuple(x.shape) != shape:
                raise ValueError(f"{name}: a float64 tensor of shape {shape} is expected")
            t = x.contiguous()
            if t.is_cuda:   # what produced the tensor on torch's current stream must be done: the shim works on the null stream
                torch.cuda.current_stream(t.device).synchronize()
            # (a host tensor, or one on another device, goes to the device entry all the same: the shim refuses it)
            _check(getattr(self.shim, symbol)(self.handle, _ptr(t), shape[0]), symbol)
            return t
        a = np.ascontiguousarray(x, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"{name}: shape {shape} is expected, not {a.shape}")
        _check(getattr(self.shim, symbol + "_host")(self.handle, a.ctypes.data, shape[0]), symbol + "_host")
        return a

    def bvh_cost(self):
        """the expected walk cost of the scene's current tree (refitted, if it was), evaluated on the device by the fixed
        reduction tree rt_hip.h states (rt_hip_scene_bvh_cost): 8 bytes come back, not the nodes"""
        cost = C.c_double(0)
        _check(self.shim.rt_hip_scene_bvh_cost(self.handle, C.byref(cost)), "rt_hip_scene_bvh_cost")
        return cost.value

    def rebuild_bvh(self):
        """Rebuilds the triangle hierarchy in place with the device builder, over the triangles as they are now
        (rt_hip_scene_rebuild_bvh): afterwards tree, kernel_name(), frames, bytes, counters and queries equal those of
        GpuScene(..., bvh="device") created from the same positions.  Handles stay; open accumulations refuse it."""
        _check(self.shim.rt_hip_scene_rebuild_bvh(self.handle), "rt_hip_scene_rebuild_bvh")

    def rebuild_info(self):
        """{"rebuilds", "last_seconds", "built_cost": bvh_cost() of the tree as it was last built}"""
        k, s, c = C.c_uint64(0), C.c_double(0), C.c_double(0)
        _check(self.shim.rt_hip_scene_rebuild_info(self.handle, C.byref(k), C.byref(s), C.byref(c)), "rt_hip_scene_rebuild_info")
        return {"rebuilds": k.value, "last_seconds": s.value, "built_cost": c.value}

    def maintain_bvh(self, max_ratio):
        """Prices the current tree on the device and rebuilds it in place iff bvh_cost() / built_cost > max_ratio (finite, >= 1)
        -> {"cost_ratio", "rebuilt"} (rt_hip_scene_maintain_bvh)"""
        ratio, rebuilt = C.c_double(0), C.c_int(0)
        _check(self.shim.rt_hip_scene_maintain_bvh(self.handle, float(max_ratio), C.byref(ratio), C.byref(rebuilt)),
               "rt_hip_scene_maintain_bvh")
        return {"cost_ratio": ratio.value, "rebuilt": bool(rebuilt.value)}

    def spheres(self):
        """the scene's spheres as they are now: a float64 (n_objects, 4) device tensor, cx cy cz radius in object order -- what the
        scene was created from, or the last update_spheres() made THROUGH THIS OBJECT (a clone of its input: the scene itself keeps
        r * r, not the radius, so they cannot be read back).  A caller that updates through the C ABI directly keeps its own copy:
        this one does not see that update.  What Temporal.frame(prev_spheres=...) takes as "now".  Not to be written."""
        if getattr(self, "_spheres", None) is None:
            a = np.array([[o.center.x, o.center.y, o.center.z, o.radius] for o in self.scene.objects[:self.scene.n_objects]],
                         dtype=np.float64).reshape(-1, 4)
            self._spheres = torch.from_numpy(a).to(self.dev)
        return self._spheres

    def update_spheres(self, spheres):
        """Moves the scene's spheres in place (rt_hip.h, rt_hip_scene_update_spheres): centre and radius of EVERY sphere, shape
        (n_objects, 4) -- cx cy cz radius, in object order -- as a float64 torch tensor on the scene's device (taken where it lies)
        or a numpy array (staged by the shim).  Synchronous.  Records, derived scalars, kernel_name(), frames, bytes and counters
        equal a freshly created scene's.  A Temporal keeps its history across the move when its next frame() is given the spheres
        from before it (prev_spheres).  Open accumulations refuse the update.  self.scene keeps the spheres the scene was created
        from; spheres() has the current ones."""
        x = self._update("update_spheres", spheres, (self.scene.n_objects, 4))
        self._spheres = x.detach().clone() if isinstance(x, torch.Tensor) else torch.from_numpy(x.copy()).to(self.dev)

    def read_spheres(self):
        """for tests: dict of numpy arrays as the kernels read them -- entry (n, 6: cx cy cz r^2 |c| 0), geom4 (n, 4)"""
        n = self.scene.n_objects
        out = dict(entry=np.zeros((n, 6)), geom4=np.zeros((n, 4)))
        _check(self.shim.rt_hip_scene_read_spheres(self.handle, *[out[k].ctypes.data if n else None for k in ("entry", "geom4")]),
               "rt_hip_scene_read_spheres")
        return out

    def sphere_bounds(self):
        """for tests: what the scene derives from its spheres -- {"reach_spheres", "max_center", "wide_range", "n_big", "big_r",
        "big_c"} (the last two: tuples of 8, zero from n_big on)"""
        reach, mc, wide, nb = C.c_double(0), C.c_double(0), C.c_uint32(0), C.c_uint32(0)
        br, bc = (C.c_double * 8)(), (C.c_double * 8)()
        _check(self.shim.rt_hip_scene_sphere_bounds(self.handle, C.byref(reach), C.byref(mc), C.byref(wide), C.byref(nb), C.byref(br),
                                                    C.byref(bc)), "rt_hip_scene_sphere_bounds")
        return {"reach_spheres": reach.value, "max_center": mc.value, "wide_range": bool(wide.value), "n_big": nb.value,
                "big_r": tuple(br), "big_c": tuple(bc)}

    def materials(self):
        """the scene's materials as they are now: (colors float64 (n, 3), emission float64 (n, 3), flags int32 (n,)) device
        tensors, n = n_objects + n_meshes in the shim's numbering (spheres, then mesh m at n_objects + m) -- what the scene was
        created from, or the last update_materials() made THROUGH THIS OBJECT.  Not to be written."""
        if getattr(self, "_materials", None) is None:
            sc = self.scene
            things = [sc.objects[i] for i in range(sc.n_objects)] + [sc.meshes[m] for m in range(sc.n_meshes)]
            a = np.array([o.color.tuple() + o.emission.tuple() for o in things], dtype=np.float64).reshape(-1, 6)
            f = np.array([o.flags for o in things], dtype=np.int32).reshape(-1)
            a, f = torch.from_numpy(a).to(self.dev), torch.from_numpy(f).to(self.dev)
            self._materials = (a[:, :3].contiguous(), a[:, 3:].contiguous(), f)
        return self._materials

    def update_materials(self, colors=None, emission=None, flags=None):
        """Changes the scene's materials in place (rt_hip.h, rt_hip_scene_update_materials): colors and emission of shape (n, 3),
        n = n_objects + n_meshes -- spheres in object order, then mesh m at n_objects + m -- as float64 torch tensors on the
        scene's device or numpy arrays; flags of shape (n,), int32 / uint32 (abi.M_*).  An omitted part keeps its current values
        (flags: the scene's own records keep theirs).  With every part given as a tensor the device entry reads them where they
        lie; otherwise the host entry stages them.  Synchronous.  Records, derived scalars, kernel names, frames, bytes and
        counters equal a freshly created scene's; geometry, tables and every handle stay.  A Temporal or a Preview holds radiance
        of the old materials: reset it after an update.  Open accumulations refuse the update.  self.scene keeps the materials the
        scene was created from; materials() has the current ones.  (_update's body takes one array and one pointer; here up to three
        parts, each given or kept, decide together which entry is taken, so the dispatch is this method's own.)"""
        n = self.scene.n_objects + self.scene.n_meshes
        col0, emi0, flg0 = self.materials()
        parts = [col0 if colors is None else colors, emi0 if emission is None else emission]
        for name, x in zip(("colors", "emission"), parts):
            if isinstance(x, torch.Tensor) and x.dtype != torch.float64 or tuple(x.shape) != (n, 3):
                raise ValueError(f"update_materials: {name} of shape {(n, 3)} (float64 where a tensor) are expected")
        if flags is not None:
            if (flags.dtype not in ((torch.int32, torch.uint32) if isinstance(flags, torch.Tensor) else (np.dtype(np.int32), np.dtype(np.uint32)))
                    or tuple(flags.shape) != (n,)):
                raise ValueError(f"update_materials: flags of shape {(n,)}, int32 or uint32, are expected")
        if all(isinstance(x, torch.Tensor) for x in parts) and isinstance(flags, (torch.Tensor, type(None))):
            # the device entry: one (n, 6) tensor of the two parts (a host tensor goes down all the same: the shim refuses it)
            t = torch.cat([x.to(torch.float64) for x in parts], dim=1).contiguous()
            f = None if flags is None else flags.contiguous()
            for x in (t, f):
                if x is not None and x.is_cuda:   # what produced it on torch's current stream must be done: the shim works on the null stream
                    torch.cuda.current_stream(x.device).synchronize()
            _check(self.shim.rt_hip_scene_update_materials(self.handle, _ptr(t), _ptr(f), n), "rt_hip_scene_update_materials")
            new_f = flg0 if f is None else f.detach().view(torch.int32).clone().to(self.dev)
        else:
            host = [x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x for x in parts]
            a = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64) for x in host], axis=1))
            f = None if flags is None else np.ascontiguousarray(flags.detach().cpu().numpy() if isinstance(flags, torch.Tensor) else flags)
            _check(self.shim.rt_hip_scene_update_materials_host(self.handle, a.ctypes.data, None if f is None else f.ctypes.data, n),
                   "rt_hip_scene_update_materials_host")
            t = torch.from_numpy(a).to(self.dev)
            new_f = flg0 if f is None else torch.from_numpy(f.astype(np.int32)).to(self.dev)
        self._materials = (t[:, :3].contiguous(), t[:, 3:].contiguous(), new_f)

    def read_materials(self):
        """for tests: dict of numpy arrays as the kernels read them -- material (n, 8: prob, albedo / prob, emission, the flags as
        the bit pattern of column 7), color_raw (n, 3)"""
        n = self.scene.n_objects + self.scene.n_meshes
        out = dict(material=np.zeros((n, 8)), color_raw=np.zeros((n, 3)))
        _check(self.shim.rt_hip_scene_read_materials(self.handle, *[out[k].ctypes.data if n else None for k in ("material", "color_raw")]),
               "rt_hip_scene_read_materials")
        return out

    def material_bounds(self):
        """for tests: what the scene derives from its materials -- {"max_emission", "any_refract", "any_checker",
        "any_mirror_glass"}"""
        e, r, c, g = C.c_double(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(self.shim.rt_hip_scene_material_bounds(self.handle, C.byref(e), C.byref(r), C.byref(c), C.byref(g)),
               "rt_hip_scene_material_bounds")
        return {"max_emission": e.value, "any_refract": bool(r.value), "any_checker": bool(c.value), "any_mirror_glass": bool(g.value)}

    def update_info(self):
        """{"updates": how many update_vertices(), update_spheres() and update_materials() the scene has taken, "last_seconds": the
        host-clock time of the last}"""
        k, s = C.c_uint64(0), C.c_double(0)
        _check(self.shim.rt_hip_scene_update_info(self.handle, C.byref(k), C.byref(s)), "rt_hip_scene_update_info")
        return {"updates": k.value, "last_seconds": s.value}

    def read_triangles(self):
        """for tests: dict of numpy arrays as the kernels read them -- geom (n, 9: v0, e1, e2), normal (n, 3), entry (n, 6: the
        phase-1 bound), object (n, uint32: material slot and hull bits)"""
        n = self.scene.n_triangles
        out = dict(geom=np.zeros((n, 9)), normal=np.zeros((n, 3)), entry=np.zeros((n, 6)), object=np.zeros(n, dtype=np.uint32))
        _check(self.shim.rt_hip_scene_read_triangles(self.handle, *[out[k].ctypes.data if n else None
                                                                    for k in ("geom", "normal", "entry", "object")]),
               "rt_hip_scene_read_triangles")
        return out

    def bounds(self):
        """for tests: {"mesh_center", "mesh_radius" (< 0: no triangles), "reach", "mesh_round"}"""
        c, r, reach, rnd = (C.c_double * 3)(), C.c_double(0), C.c_double(0), C.c_uint32(0)
        _check(self.shim.rt_hip_scene_bounds(self.handle, C.byref(c), C.byref(r), C.byref(reach), C.byref(rnd)), "rt_hip_scene_bounds")
        return {"mesh_center": tuple(c), "mesh_radius": r.value, "reach": reach.value, "mesh_round": bool(rnd.value)}

    def suggest_chunks(self, count, samples=None, max_depth=None):
        return int(self.shim.rt_hip_suggest_chunks_depth(self.handle, count, samples or self.scene.samples,
                                                         _depth(self.scene, max_depth)))

    def render_tiles(self, seed, first, stride, count, tiles=None, tiles8=None, stats=None, samples=None,
                     max_depth=None, chunks=1, workspace=None, integrator="path", camera=None):
        """Asynchronous on torch's current stream.  Returns (tiles f32 [count,64,3],
        tiles8 u8 [count,64,3], stats i64 [4]); pass buffers to reuse them.  chunks > 1 splits
        every tile's samples over that many workgroups (same image, bit for bit).
        integrator: "path" = trace_path (what the reference ships), "whitted" = cast_ray.
        camera: an abi.Camera to render with instead of the scene's own."""
        dev = self.dev
        if tiles is None:
            tiles = torch.empty((max(count, 1), abi.TILE_PIXELS, 3), dtype=torch.float32, device=dev)
        if tiles8 is None:
            tiles8 = torch.empty((max(count, 1), abi.TILE_PIXELS, 3), dtype=torch.uint8, device=dev)
        stats = _counters(dev, stats)
        p = self.params(seed, first, stride, count, samples, max_depth, integrator)
        if chunks > 1 and workspace is None:
            workspace = torch.empty(self.shim.rt_hip_scene_chunk_workspace_bytes(self.handle, max(count, 1)), dtype=torch.uint8, device=dev)
        self._workspace = workspace  # keep alive until the stream has used it
        _check(self.shim.rt_hip_render_tiles_chunked(self.handle, C.byref(_camera(self.scene, camera)), C.byref(p), chunks,
                                                     workspace.data_ptr() if workspace is not None else None,
                                                     tiles.data_ptr(), tiles8.data_ptr(), stats.data_ptr(),
                                                     _stream(dev)),
               "rt_hip_render_tiles_chunked")
        return tiles, tiles8, stats

    def accumulate(self, seed, samples, max_depth=None, integrator="path", first=0, stride=1, count=None, camera=None):
        """A progressive render of `samples` per pixel (the budget) over tiles first + k * stride, k < count (default: the whole
        image), added in passes: Accumulation.add(n).  After the whole budget its resolve() is render_tiles()' frame for the same
        budget at suggest_chunks() chunks, bit for bit, whatever the passes were (rt_hip.h, rt_hip_accum_*)."""
        if count is None:
            count = n_tiles(self.scene.width, self.scene.height)
        p = self.params(seed, first, stride, count, samples, max_depth, integrator)
        handle = C.c_void_p()
        _check(self.shim.rt_hip_accum_create(self.handle, C.byref(_camera(self.scene, camera)), C.byref(p), C.byref(handle)),
               "rt_hip_accum_create")
        self._accums = [h for h in self._accums if h] + [handle]
        return Accumulation(self, handle, count, seed, first, stride, camera)

    def untile(self, tiles, tiles8, first, stride, count, image=None, image8=None):
        """Scatter a compact tile buffer into row-major images on torch's current stream."""
        dev = tiles.device
        w, h = self.scene.width, self.scene.height
        if image is None:
            image = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        if image8 is None and tiles8 is not None:
            image8 = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
        _check(self.shim.rt_hip_untile(tiles.data_ptr(), tiles8.data_ptr() if tiles8 is not None else None, w, h,
                                       first, stride, count, image.data_ptr(),
                                       image8.data_ptr() if image8 is not None else None, _stream(dev)),
               "rt_hip_untile")
        return image, image8

    def aov_kernel_name(self):
        """the AOV form this scene's render_aov launches take"""
        return self.shim.rt_hip_aov_kernel_name(self.handle).decode()

    def render_aov(self, seed, samples, first=0, stride=1, count=None, camera=None, want=abi.AOV_FIELDS):
        """First-hit feature buffers of `samples` camera samples per pixel (rt_hip.h, rt_hip_render_aov_tiles) over tiles
        first + k * stride, k < count (default: the whole image), asynchronous on torch's current stream -> dict of compact
        tile-major tensors: albedo / normal f32 [count,64,3], depth f32 [count,64], object / hits int32 [count,64] (the uint32
        words of the C-ABI, bit for bit: .view(torch.uint32) or numpy's .view(np.uint32) reads them as such).  want: which."""
        if count is None:
            count = n_tiles(self.scene.width, self.scene.height)
        dev = self.dev
        out = {f: torch.empty(_aov_shape(f, max(count, 1), abi.TILE_PIXELS), dtype=_TORCH[abi.AOV_DTYPES[f]], device=dev) for f in want}
        p = self.params(seed, first, stride, count, samples)
        _check(self.shim.rt_hip_render_aov_tiles(self.handle, C.byref(_camera(self.scene, camera)), C.byref(p),
                                                 C.byref(_aov_record(out, want)), _stream(dev)), "rt_hip_render_aov_tiles")
        return out

    def untile_aov(self, tiles, first, stride, count):
        """Scatter render_aov's compact buffers into row-major tensors ([H,W,3] / [H,W], zeros where no tile of the set lies)
        on torch's current stream"""
        w, h = self.scene.width, self.scene.height
        out = {f: torch.zeros(_aov_shape(f, h, w), dtype=t.dtype, device=t.device) for f, t in tiles.items()}
        return self._untile_aov(tiles, first, stride, count, out)

    def _untile_aov(self, tiles, first, stride, count, out):
        """... into the row-major tensors `out` holds for the tiles' fields"""
        _check(self.shim.rt_hip_untile_aov(C.byref(_aov_record(tiles, tiles)), self.scene.width, self.scene.height, first, stride, count,
                                           C.byref(_aov_record(out, tiles)), _stream(self.dev)), "rt_hip_untile_aov")
        return out

    def aov_image(self, seed, samples):
        """The whole image's feature buffers on this GPU, synchronised -> dict of row-major numpy arrays: albedo / normal
        float32 [H,W,3], depth float32 [H,W], object / hits uint32 [H,W]"""
        total = n_tiles(self.scene.width, self.scene.height)
        img = self.untile_aov(self.render_aov(seed, samples, 0, 1, total), 0, 1, total)
        torch.cuda.synchronize(self.dev)
        return {f: t.cpu().numpy().view(abi.AOV_DTYPES[f]) for f, t in img.items()}

    def query_kernel_name(self):
        """the ray-query form this scene's query_rays / query_uv launches take"""
        return self.shim.rt_hip_query_kernel_name(self.handle).decode()

    def _query(self, rays, per_ray, t_max, params, want, into=None):
        dev = self.dev
        rays = _device_rays(rays, per_ray, dev)
        n = rays.shape[0]
        if t_max is not None:
            t_max = torch.as_tensor(t_max, dtype=torch.float64, device=dev).reshape(-1).contiguous()
            if t_max.numel() != n:
                raise ValueError("query: t_max must hold one value per ray")
        out, hits = _wanted(abi.RtHipHits(), abi.HIT_SHAPES, want, n, dev, into=into)
        self._query_inputs = (rays, t_max)   # keep alive until the stream has used them
        _check(self.shim.rt_hip_query_rays(self.handle, _some(rays), _ptr(t_max) if n else None, n, C.byref(params),
                                           C.byref(hits), _stream(dev)), "rt_hip_query_rays")
        return out

    def query_rays(self, rays, t_max=None, normalize=False, origin_radius=None, want=abi.HIT_FIELDS):
        """Closest hits of the caller's rays (rt_hip.h, rt_hip_query_rays): rays [n, 6] float64 (origin, direction; a tensor on the
        scene's device or anything torch.as_tensor takes), t_max [n] or None, asynchronous on torch's current stream -> dict of
        device tensors: status / object / prim int32 [n] (the uint32 words of the C-ABI: numpy's .view(np.uint32) reads them as
        such), t float64 [n], point / normal [n, 3], bary [n, 2], ray [n, 6].  want: which.  origin_radius: how far from the world
        origin the rays start (a speed hint that changes no output bit; None: the default)."""
        return self._query(rays, 6, t_max, abi.query_params(abi.RAYS_GIVEN, normalize, None, origin_radius), want)

    def query_uv(self, uv, camera=None, t_max=None, normalize=False, origin_radius=None, want=abi.HIT_FIELDS, out=None):
        """... of the camera rays get_camera_ray(camera, u, v) for uv [n, 2] float64 (camera None: the scene's own; origin_radius
        None: the camera's distance from the world origin; out: a dict of tensors to write wanted fields into, what is missing
        is allocated)"""
        cam, origin_radius = self._uv_source(camera, origin_radius)
        return self._query(uv, 2, t_max, abi.query_params(abi.RAYS_CAMERA_UV, normalize, cam, origin_radius), want, out)

    def _uv_source(self, camera, origin_radius):
        """(camera, origin_radius) of a query of camera rays: the scene's own camera, and its distance from the world's origin"""
        cam = _camera(self.scene, camera)
        return cam, _distance(cam.position.tuple()) if origin_radius is None else origin_radius

    def pick(self, x, y):
        """What is under the centre of pixel (x, y) of the scene's own camera and size: u = (x + 0.5) / (w - 1), v = (y + 0.5) /
        (h - 1) -> dict of Python values: status, object, prim, t, point, normal (synchronises)"""
        uv = [[(x + 0.5) / (self.scene.width - 1), (y + 0.5) / (self.scene.height - 1)]]
        out = self.query_uv(uv, want=("status", "object", "prim", "t", "point", "normal"))
        torch.cuda.synchronize(self.dev)
        res = {f: t.cpu().numpy() for f, t in out.items()}
        return dict(status=int(res["status"][0]), object=int(res["object"].view("uint32")[0]), prim=int(res["prim"].view("uint32")[0]),
                    t=float(res["t"][0]), point=tuple(res["point"][0].tolist()), normal=tuple(res["normal"][0].tolist()))

    def trace_kernel_name(self):
        """the radiance-query form this scene's trace_rays / trace_uv launches take"""
        return self.shim.rt_hip_trace_kernel_name(self.handle).decode()

    def _trace(self, rays, per_ray, params, want, stats):
        dev = self.dev
        rays = _device_rays(rays, per_ray, dev)
        n = rays.shape[0]
        out, rad = self._radiance(want, n, params.samples, stats)
        self._trace_inputs = rays   # keep alive until the stream has used them
        _check(self.shim.rt_hip_trace_rays(self.handle, _some(rays), n, C.byref(params), C.byref(rad), _ptr(out["stats"]), _stream(dev)),
               "rt_hip_trace_rays")
        return out

    def _radiance(self, want, n, samples, stats):
        """(dict, RtHipRadiance) of a radiance query's outputs `want` for n entries, the counters -- given or zeros -- as out["stats"]"""
        out, rad = _wanted(abi.RtHipRadiance(), abi.RADIANCE_SHAPES, want, n, self.dev, samples)
        out["stats"] = _counters(self.dev, stats)
        return out, rad

    def trace_rays(self, rays, samples, seed, max_depth=None, normalize=False, origin_radius=None, index_first=0,
                   want=("status", "radiance"), stats=None):
        """What light arrives along the caller's rays (rt_hip.h, rt_hip_trace_rays): rays [n, 6] float64 (origin, direction), the
        mean of `samples` trace_path samples per ray, sample s of ray i on the stream (seed, index_first + i, s); asynchronous on
        torch's current stream -> dict of device tensors: status int32 [n] (the uint32 words of the C-ABI), radiance float64
        [n, 3], samples [n, samples, 3], paths / casts int64 [n], ray [n, 6] (want: which), and stats int64 [4] (rays, casts, tests,
        samples; += into the tensor given).  max_depth None: the scene's own."""
        p = abi.trace_params(samples, seed, _depth(self.scene, max_depth), abi.RAYS_GIVEN, normalize, None, origin_radius, index_first)
        return self._trace(rays, 6, p, want, stats)

    def trace_uv(self, uv, samples, seed, camera=None, max_depth=None, normalize=False, origin_radius=None, index_first=0,
                 want=("status", "radiance"), stats=None):
        """... of the camera rays get_camera_ray(camera, u, v) for uv [n, 2] float64 (camera None: the scene's own; origin_radius
        None: the camera's distance from the world origin)"""
        cam, origin_radius = self._uv_source(camera, origin_radius)
        p = abi.trace_params(samples, seed, _depth(self.scene, max_depth), abi.RAYS_CAMERA_UV, normalize, cam, origin_radius, index_first)
        return self._trace(uv, 2, p, want, stats)

    def pixel_kernel_name(self):
        """the pixel-refinement form this scene's trace_pixels launches take"""
        return self.shim.rt_hip_pixel_kernel_name(self.handle).decode()

    def trace_pixels(self, pixels, samples, seed, sample_first=0, camera=None, max_depth=None, n=None, want=("status", "radiance"),
                     stats=None):
        """render()'s own samples sample_first .. sample_first + samples - 1 of the listed pixels of the scene's frame (rt_hip.h,
        rt_hip_trace_pixels): pixels the uint32 indices y * width + x (a 32-bit tensor on the scene's device, as select_pixels
        returns it, or anything numpy takes), n: how many of them to trace (None: all); asynchronous on torch's current stream ->
        dict of device tensors: status int32 [n], radiance float64 [n, 3], samples [n, samples, 3], paths / casts int64 [n] (want:
        which), and stats int64 [4] (+= into the tensor given).  camera None: the scene's own; max_depth None: the scene's own."""
        dev = self.dev
        pixels = _pixel_tensor(pixels, dev)
        n = pixels.numel() if n is None else int(n)
        if n < 0 or n > pixels.numel():
            raise ValueError("trace_pixels(): n must be within the list")
        p = abi.pixel_params(self.scene.width, self.scene.height, samples, seed, sample_first, _depth(self.scene, max_depth))
        for f in want:
            if f not in abi.PIXEL_FIELDS:
                raise ValueError(f"trace_pixels(): {f!r} is not an output of a pixel refinement")
        out, rad = self._radiance(want, n, samples, stats)
        self._pixel_inputs = pixels   # keep alive until the stream has used them
        _check(self.shim.rt_hip_trace_pixels(self.handle, C.byref(_camera(self.scene, camera)), _some(pixels, n), n, C.byref(p), C.byref(rad),
                                             _ptr(out["stats"]), _stream(dev)), "rt_hip_trace_pixels")
        return out

    def refine(self, rgb, values, lo, hi, samples, seed, sample_first=0, prior=None, prior_scale=0.0, invert=False, camera=None,
               max_depth=None, rgb8=None, weight=None, stats=None):
        """Select, trace, blend, on torch's current stream: the pixels of `values` (f32 [H,W]) within [lo, hi] (select_pixels) get
        `samples` more samples of the render's own from sample_first on (trace_pixels) and are blended into rgb (f32 [H,W,3], in
        place) with new_weight = samples against prior_scale * prior (blend_pixels; prior_scale 0: replaced).  rgb8, weight: updated
        at the touched pixels when given.  -> the number of pixels selected (waits for that one word)."""
        w, h = self.scene.width, self.scene.height
        idx, count = select_pixels(values, w, h, lo, hi, invert=invert)
        if count:
            out = self.trace_pixels(idx, samples, seed, sample_first, camera, max_depth, n=count, stats=stats)
            blend_pixels(idx, out["status"], out["radiance"], rgb, w, h, float(samples), prior_scale, prior=prior, rgb8=rgb8, weight=weight,
                         n=count)
        return count

    def render_lens(self, aperture, focus, samples, seed, camera=None, max_depth=None, slice_pixels=None, stats=None):
        """A frame with depth of field (rt_hip.h, rt_hip_render_lens): a thin lens of radius `aperture` focused at distance `focus`
        in front of the camera (None: the scene's own), `samples` lens rays per pixel traced by the radiance query; asynchronous on
        torch's current stream -> (rgb float32 [H, W, 3], rgb8 uint8 [H, W, 3], sum float64 [H, W, 3], stats int64 [4]; += into the
        tensor given).  slice_pixels: pixels per launch (None: the whole frame); no output bit depends on it."""
        dev = self.dev
        w, h = self.scene.width, self.scene.height
        p = self.params(seed, 0, 0, 0, samples=samples, max_depth=max_depth)
        lens = abi.lens_params(aperture, focus)
        slice_pixels = w * h if slice_pixels is None else slice_pixels
        ws = _workspace(self.shim.rt_hip_lens_workspace_bytes(w, h, slice_pixels), dev)
        rgb, rgb8 = _frame_pair(h, w, dev)
        total = torch.empty((h, w, 3), dtype=torch.float64, device=dev)
        stats = _counters(dev, stats)
        self._lens_workspace = ws   # keep alive until the stream has used it
        _check(self.shim.rt_hip_render_lens(self.handle, C.byref(_camera(self.scene, camera)), C.byref(lens), C.byref(p), slice_pixels, _ptr(ws),
                                            _ptr(total), _ptr(rgb), _ptr(rgb8), _ptr(stats), _stream(dev)), "rt_hip_render_lens")
        return rgb, rgb8, total, stats

    def focus_at(self, x, y, camera=None):
        """Autofocus: the focus_distance that puts what is under the centre of pixel (x, y) in focus, or None where the ray misses.
        One ray query through the pixel centre (as pick()); the hit's t over |d|, d the lens contract's direction, not normalised:
        d = position - (lower_left_corner + (horizontal*u + vertical*v)) (synchronises)"""
        cam = _camera(self.scene, camera)
        u, v = (x + 0.5) / (self.scene.width - 1.0), (y + 0.5) / (self.scene.height - 1.0)
        out = self.query_uv([[u, v]], camera=cam, want=("status", "t"))
        torch.cuda.synchronize(self.dev)
        if int(out["status"].cpu()[0]) != 1:
            return None
        pos, llc, hor, ver = (c.tuple() for c in (cam.position, cam.lower_left_corner, cam.horizontal, cam.vertical))
        d = [pos[k] - (llc[k] + (hor[k] * u + ver[k] * v)) for k in range(3)]
        return float(out["t"].cpu()[0]) / ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) ** 0.5

    def _bake(self, mode, positions, normals, samples, seed, bias, max_depth, origin_radius, slice_rays, stats):
        """rt_hip_bake_probes on torch's current stream -> dict(coeff float64 [N, bases, 3], coeff_f float32, sum float64, status int32
        [N], stats int64 [4])"""
        dev = self.dev
        pos, nrm = _points3(positions, dev), None if normals is None else _points3(normals, dev)
        n, bases = pos.shape[0], abi.PROBE_BASES[mode]
        if nrm is not None and nrm.shape[0] != n:
            raise ValueError(f"{nrm.shape[0]} normals for {n} probes")
        if origin_radius is None:
            norms = lambda t: None if t is None else torch.linalg.vector_norm(t, dim=1)
            origin_radius = _origin_radius(norms(pos), norms(nrm), bias)   # (synchronises)
        p = abi.probe_params(mode, samples, seed, _depth(self.scene, max_depth), bias, origin_radius)
        slice_rays, launch = _slices(n, samples, slice_rays)
        ws = _workspace(self.shim.rt_hip_probe_workspace_bytes(n, mode, launch), dev)
        out = dict(coeff=torch.empty((n, bases, 3), dtype=torch.float64, device=dev),
                   coeff_f=torch.empty((n, bases, 3), dtype=torch.float32, device=dev),
                   sum=torch.empty((n, bases, 3), dtype=torch.float64, device=dev), status=torch.empty(n, dtype=torch.int32, device=dev),
                   stats=_counters(dev, stats))
        self._probe_buffers = (ws, pos, nrm)   # keep alive until the stream has used them
        _check(self.shim.rt_hip_bake_probes(self.handle, _some(pos), _some(nrm), n, C.byref(p), slice_rays, _ptr(ws), _some(out["sum"]),
                                            _some(out["coeff"]), _some(out["coeff_f"]), _some(out["status"]), _ptr(out["stats"]), _stream(dev)),
               "rt_hip_bake_probes")
        return out

    def bake_probes(self, positions, samples, seed, max_depth=None, origin_radius=None, slice_rays=None, stats=None, details=False):
        """Light probes (rt_hip.h, rt_hip_bake_probes, RT_HIP_PROBE_SPHERE): the SH9 coefficients of the radiance arriving at
        positions [N, 3] from `samples` uniform directions a probe, traced by the radiance query; asynchronous on torch's current
        stream -> float64 [N, 9, 3] on the device (details: the dict of coeff, coeff_f float32, sum, status int32 [N] -- 2 where a
        ray of the probe was invalid --, stats).  origin_radius None: the largest finite |position| (synchronises); slice_rays: rays
        per launch (None: all); no output bit depends on either."""
        out = self._bake(abi.PROBE_SPHERE, positions, None, samples, seed, 0.0, max_depth, origin_radius, slice_rays, stats)
        return out if details else out["coeff"]

    def bake_irradiance(self, positions, normals, samples, seed, bias=0.0, max_depth=None, origin_radius=None, slice_rays=None, stats=None,
                        details=False):
        """Irradiance at surface points (rt_hip.h, rt_hip_bake_probes, RT_HIP_PROBE_HEMISPHERE): E = 2 pi x the mean of radiance x
        cosine over `samples` uniform directions of the hemisphere about normals [N, 3] (used as given), rays starting at position +
        normal * bias -> float64 [N, 3] on the device (details: as bake_probes, the arrays [N, 1, 3])"""
        out = self._bake(abi.PROBE_HEMISPHERE, positions, normals, samples, seed, bias, max_depth, origin_radius, slice_rays, stats)
        return out if details else out["coeff"].reshape(-1, 3)

    def bake_probe_grid(self, grid, samples, seed, max_depth=None, origin_radius=None, slice_rays=None, stats=None, details=False, vis=None):
        """A grid of sphere probes baked in one call (rt_hip.h, rt_hip_bake_probe_grid: the grid's positions, then rt_hip_bake_probes
        at them); grid: abi.probe_grid(...) -> float64 [N, 9, 3] on the device, N = the grid's probes in index order (details: the dict
        of coeff, coeff_f, status, stats).  origin_radius None: the farthest corner of the grid from the world's origin.  vis
        (abi.probe_vis(...)): the depth moments of the same rays as well (rt_hip_bake_probe_grid_depth) -> (coeff, moments float64
        [N, R*R, 2]); details: the dict gains moments and depth_status."""
        dev, n = self.dev, _grid_count(grid)
        p = abi.probe_params(abi.PROBE_SPHERE, samples, seed, _depth(self.scene, max_depth), 0.0,
                             _grid_radius(grid) if origin_radius is None else origin_radius)
        slice_rays, launch = _slices(n, samples, slice_rays)
        ws = _workspace(self.shim.rt_hip_probe_grid_workspace_bytes(C.byref(grid), launch), dev)
        out = dict(coeff=torch.empty((n, 9, 3), dtype=torch.float64, device=dev), coeff_f=torch.empty((n, 9, 3), dtype=torch.float32, device=dev),
                   status=torch.empty(n, dtype=torch.int32, device=dev), stats=_counters(dev, stats))
        self._probe_buffers = (ws,)   # keep alive until the stream has used them
        _check(self.shim.rt_hip_bake_probe_grid(self.handle, C.byref(grid), C.byref(p), slice_rays, _ptr(ws), _ptr(out["coeff"]), _ptr(out["coeff_f"]),
                                                _ptr(out["status"]), _ptr(out["stats"]), _stream(dev)), "rt_hip_bake_probe_grid")
        if vis is not None:
            out["moments"], out["depth_status"] = self._grid_depth(grid, vis, p, slice_rays, launch)
            return out if details else (out["coeff"], out["moments"])
        return out if details else out["coeff"]

    def _grid_depth(self, grid, vis, p, slice_rays, launch):
        """rt_hip_bake_probe_grid_depth under the probe params p -> (moments float64 [N, R*R, 2], status int32 [N])"""
        dev, n = self.dev, _grid_count(grid)
        ws = _workspace(self.shim.rt_hip_probe_grid_depth_workspace_bytes(C.byref(grid), vis.res, launch), dev)
        moments = torch.empty((n, vis.res * vis.res, 2), dtype=torch.float64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        self._depth_buffers = (ws,)   # keep alive until the stream has used them
        _check(self.shim.rt_hip_bake_probe_grid_depth(self.handle, C.byref(grid), C.byref(vis), C.byref(p), slice_rays, _ptr(ws), _ptr(moments),
                                                      _ptr(status), _stream(dev)), "rt_hip_bake_probe_grid_depth")
        return moments, status

    def probe_depth_moments(self, positions, vis, samples, seed, origin_radius=None, slice_rays=None, details=False):
        """The depth moments of sphere probes at positions [N, 3] (rt_hip.h, rt_hip_bake_probe_depth): per probe an R x R octahedral
        map of the mean and the mean square of the distance to the nearest surface, folded from the closest hits of the very rays
        bake_probes traces under the same samples and seed; vis: abi.probe_vis(...); asynchronous on torch's current stream ->
        float64 [N, R*R, 2] on the device (details: the dict of moments and status int32 [N], 2 where a ray of the probe was
        invalid).  positions may be an abi.probe_grid(...): the grid's probes (rt_hip_bake_probe_grid_depth).  No output bit depends
        on origin_radius or slice_rays."""
        dev = self.dev
        if isinstance(positions, abi.RtHipProbeGrid):
            grid = positions
            p = abi.probe_params(abi.PROBE_SPHERE, samples, seed, None, 0.0, _grid_radius(grid) if origin_radius is None else origin_radius)
            slice_rays, launch = _slices(_grid_count(grid), samples, slice_rays)
            moments, status = self._grid_depth(grid, vis, p, slice_rays, launch)
            return dict(moments=moments, status=status) if details else moments
        pos = _points3(positions, dev)
        n = pos.shape[0]
        if origin_radius is None:
            origin_radius = _origin_radius(torch.linalg.vector_norm(pos, dim=1), None, 0.0)   # (synchronises)
        p = abi.probe_params(abi.PROBE_SPHERE, samples, seed, None, 0.0, origin_radius)
        slice_rays, launch = _slices(n, samples, slice_rays)
        ws = _workspace(self.shim.rt_hip_probe_depth_workspace_bytes(n, vis.res, launch), dev)
        moments = torch.empty((n, vis.res * vis.res, 2), dtype=torch.float64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        self._depth_buffers = (ws, pos)   # keep alive until the stream has used them
        _check(self.shim.rt_hip_bake_probe_depth(self.handle, _some(pos), n, C.byref(vis), C.byref(p), slice_rays, _ptr(ws), _some(moments),
                                                 _some(status), _stream(dev)), "rt_hip_bake_probe_depth")
        return dict(moments=moments, status=status) if details else moments

    def probe_preview(self, grid, coeff, camera=None, aov_samples=1, seed=0, vis=None, moments=None):
        """The probe-lit preview of the scene's frame (rt_hip.h, rt_hip_probe_preview): first hits at the pixel centres, their albedo
        and emission, lit by the grid's baked coefficients coeff [N, 9, 3]; asynchronous on torch's current stream ->
        (rgb float32 [H, W, 3], rgb8 uint8 [H, W, 3]) on the device.  vis (abi.probe_vis(...)) and moments [N, R*R, 2]: both or
        neither; with them the shade weighs every corner by its visibility (rt_hip_probe_preview_vis)."""
        dev = self.dev
        w, h = self.scene.width, self.scene.height
        coeff = torch.as_tensor(coeff, dtype=torch.float64, device=dev).contiguous()
        if coeff.numel() != _grid_count(grid) * 27:
            raise ValueError("probe_preview: coeff must hold 9 x 3 values per probe of the grid")
        ws = _workspace(self.shim.rt_hip_probe_preview_workspace_bytes(self.handle, w, h), dev)
        rgb, rgb8 = _frame_pair(h, w, dev)
        if (vis is None) != (moments is None):
            raise ValueError("probe_preview: vis and moments go together")
        if vis is not None:
            moments = _moments(moments, grid, vis, dev, "probe_preview")
            self._preview_buffers = (ws, coeff, moments)   # keep alive until the stream has used them
            _check(self.shim.rt_hip_probe_preview_vis(self.handle, C.byref(_camera(self.scene, camera)), C.byref(grid), C.byref(vis), _ptr(coeff),
                                                      _ptr(moments), w, h, aov_samples, seed, _ptr(ws), _ptr(rgb), _ptr(rgb8), _stream(dev)),
                   "rt_hip_probe_preview_vis")
            return rgb, rgb8
        self._preview_buffers = (ws, coeff)   # keep alive until the stream has used them
        _check(self.shim.rt_hip_probe_preview(self.handle, C.byref(_camera(self.scene, camera)), C.byref(grid), _ptr(coeff), w, h, aov_samples,
                                              seed, _ptr(ws), _ptr(rgb), _ptr(rgb8), _stream(dev)), "rt_hip_probe_preview")
        return rgb, rgb8

    def probe_grid_update(self, grid, upd, samples, seed, coeff, age, vis=None, moments=None, coeff_f=None, change=None, status=None,
                          max_depth=None, origin_radius=None, slice_rays=None, stats=None):
        """One update round of a grid's state in place (rt_hip.h, rt_hip_probe_grid_update): `samples` fresh rays for each of the
        round's probes (upd: abi.probe_update(...)), blended into coeff float64 [N, 9, 3] and -- with vis -- moments float64
        [N, R*R, 2] by each probe's age int32 [N], which steps; coeff_f float32, change float64 [N] and status int32 [N] are written
        where given.  Device tensors, asynchronous on torch's current stream -> the counters int64 [4].  No output bit depends on
        origin_radius or slice_rays."""
        dev, n = self.dev, _grid_count(grid)
        if (vis is None) != (moments is None):
            raise ValueError("probe_grid_update: vis and moments go together")
        for name, t, dt, k in (("coeff", coeff, torch.float64, 27 * n), ("age", age, torch.int32, n), ("coeff_f", coeff_f, torch.float32, 27 * n),
                               ("moments", moments, torch.float64, 0 if vis is None else 2 * n * vis.res * vis.res),
                               ("change", change, torch.float64, n), ("status", status, torch.int32, n)):
            if t is not None and not _is(t, dev, k, dt):
                raise ValueError(f"probe_grid_update: {name} must be a contiguous {dt} tensor of {k} values on the scene's device")
        p = abi.probe_params(abi.PROBE_SPHERE, samples, seed, _depth(self.scene, max_depth), 0.0,
                             _grid_radius(grid) if origin_radius is None else origin_radius)
        m = self.shim.rt_hip_probe_update_count(C.byref(grid), C.byref(upd))
        slice_rays, launch = _slices(m, samples, slice_rays)
        v = None if vis is None else C.byref(vis)
        ws = _workspace(self.shim.rt_hip_probe_update_workspace_bytes(C.byref(grid), v, C.byref(upd), launch), dev)
        stats = _counters(dev, stats)
        self._update_buffers = (ws,)   # keep alive until the stream has used them
        _check(self.shim.rt_hip_probe_grid_update(self.handle, C.byref(grid), v, C.byref(p), C.byref(upd), slice_rays, _ptr(ws), _ptr(coeff),
                                                  _ptr(coeff_f), _ptr(moments), _ptr(age), _ptr(change), _ptr(status), _ptr(stats), _stream(dev)),
               "rt_hip_probe_grid_update")
        return stats

    def probe_grid_state(self, grid, samples, seed, vis=None, hysteresis=0.9, stride=1, change=0.0, fast=0.0):
        """A grid's state that follows the scene (ProbeGridState): every age 0, nothing traced yet; .update() runs rounds of
        `samples` rays a probe under `seed`.  The state lives beside the scene, not in it: it survives update_spheres,
        update_vertices and rebuild_bvh."""
        return ProbeGridState(self, grid, samples, seed, vis, hysteresis, stride, change, fast)

    def render_panorama(self, width, height, origin, samples, seed, max_depth=None):
        """An equirectangular view from `origin` (scene.panorama_rays: no Camera expresses it), `samples` paths per pixel, pixel
        k = y * width + x on the stream (seed, k, s) -> (float64 [height, width, 3] linear radiance on the device, stats)"""
        from . import scene as S
        out = self.trace_rays(S.panorama_rays(width, height, origin), samples, seed, max_depth, origin_radius=_distance(origin),
                              want=("radiance",))
        return out["radiance"].reshape(height, width, 3), out["stats"]

    def denoised_image(self, seed, samples, **params):
        """The whole frame of `samples` per pixel (render_image), its first-hit buffers of the same samples, and the denoise
        (rt_hip_denoise; params: abi.denoise_params' keywords) -> numpy (noisy f32 [H,W,3], denoised f32 [H,W,3], denoised u8 [H,W,3])"""
        image, _, _ = self.render_image(seed, samples)
        total = n_tiles(self.scene.width, self.scene.height)
        aov = self.untile_aov(self.render_aov(seed, samples, 0, 1, total, want=DENOISE_AOV), 0, 1, total)
        rgb, rgb8 = denoise(image, aov, self.scene.width, self.scene.height, **params)
        torch.cuda.synchronize(image.device)
        return image.cpu().numpy(), rgb.cpu().numpy(), rgb8.cpu().numpy()

    def temporal(self, **params):
        """A Temporal: frames of this scene under a moving camera, each accumulated onto the reprojected history of the ones
        before (rt_hip_reproject, and rt_hip_reproject_points across update_vertices; params: abi.reproject_params' keywords)"""
        return Temporal(self, **params)

    def preview(self, scale, **params):
        """A Preview: frames of this scene rendered at ceil(width / scale) x ceil(height / scale) and brought to full size under
        the full-resolution first-hit buffers (rt_hip_upsample; scale: an integer >= 2; params: abi.upsample_params' keywords)"""
        return Preview(self, scale, **params)

    def render_adaptive(self, seed, samples, max_depth=None, integrator="path", **params):
        """An adaptive frame of at most `samples` per pixel on this GPU (Accumulation.run_adaptive; params: abi.adapt_params'
        keywords) -> (image f32 [H,W,3], image8 u8 [H,W,3], tile sample counts uint32 [tiles_y, tiles_x], stats dict, device
        seconds), synchronised."""
        w, h = self.scene.width, self.scene.height
        total = n_tiles(w, h)
        acc = self.accumulate(seed, samples, max_depth=max_depth, integrator=integrator)
        try:
            st, secs = acc.run_adaptive(**params)
            tiles, tiles8 = acc.resolve()
            image, image8 = self.untile(tiles, tiles8, 0, 1, total)
            counts = acc.tile_samples().reshape((h + abi.TILE - 1) // abi.TILE, (w + abi.TILE - 1) // abi.TILE)
            torch.cuda.synchronize(tiles.device)
            self.launch_status()
        finally:
            acc.close()
        return image, image8, counts, st, secs

    def render_image(self, seed, samples=None, max_depth=None, integrator="path"):
        """Whole image on this one GPU -> (image f32 [H,W,3], image8 u8 [H,W,3], stats dict), synchronised."""
        total = n_tiles(self.scene.width, self.scene.height)
        chunks = 1 if integrator != "path" else self.suggest_chunks(total, samples, max_depth)
        tiles, tiles8, stats = self.render_tiles(seed, 0, 1, total, samples=samples, max_depth=max_depth,
                                                 integrator=integrator, chunks=chunks)
        image, image8 = self.untile(tiles, tiles8, 0, 1, total)
        torch.cuda.synchronize(tiles.device)
        self.launch_status()   # a workgroup without its pool slot fails the frame here, not as NaN pixels
        st = stats.cpu().tolist()
        return image, image8, _stats_dict(st)


class ProbeGridState:
    """The coefficients (coeff float64 [N, 9, 3], coeff_f float32), depth moments (moments float64 [N, R*R, 2], with a vis), ages
    (age int32 [N]), last relative changes (change float64 [N]) and status words (status int32 [N]) of a grid on the scene's device,
    and the number of rounds run (round).  GpuScene.probe_grid_state() makes one."""

    def __init__(self, gs, grid, samples, seed, vis, hysteresis, stride, change, fast):
        dev, n = gs.dev, _grid_count(grid)
        self.gs, self.grid, self.vis, self.samples, self.seed = gs, grid, vis, samples, seed
        self.hysteresis, self.stride, self.change_limit, self.fast = hysteresis, stride, change, fast
        self.round = 0
        self.coeff = torch.zeros((n, 9, 3), dtype=torch.float64, device=dev)
        self.coeff_f = torch.zeros((n, 9, 3), dtype=torch.float32, device=dev)
        self.moments = None if vis is None else torch.zeros((n, vis.res * vis.res, 2), dtype=torch.float64, device=dev)
        self.age = torch.zeros(n, dtype=torch.int32, device=dev)
        self.change = torch.zeros(n, dtype=torch.float64, device=dev)
        self.status = torch.ones(n, dtype=torch.int32, device=dev)
        self.stats = _counters(dev)

    def update(self, rounds=1, slice_rays=None):
        """`rounds` update rounds: round u updates the probes of phase u % stride under the seed of round u; asynchronous"""
        for _ in range(rounds):
            upd = abi.probe_update(self.stride, self.round % self.stride, self.round & 0xFFFFFFFF, self.hysteresis, self.change_limit,
                                   self.fast)
            self.gs.probe_grid_update(self.grid, upd, self.samples, self.seed, self.coeff, self.age, self.vis, self.moments, self.coeff_f,
                                      self.change, self.status, slice_rays=slice_rays, stats=self.stats)
            self.round += 1
        return self

    def reset(self):
        """every probe starts over with its next round: the ages become 0 (the rest of the state is not read again)"""
        self.age.zero_()
        return self

    def preview(self, camera=None, aov_samples=1):
        """GpuScene.probe_preview lit by the state as it stands"""
        return self.gs.probe_preview(self.grid, self.coeff, camera, aov_samples, self.seed, self.vis, self.moments)


class Accumulation:
    """An accumulation (rt_hip_accum_*) made by GpuScene.accumulate.  Passes and resolves run asynchronously on torch's current
    stream; the scene must stay open until close()."""

    def __init__(self, gs, handle, count, seed=None, first=0, stride=1, camera=None):
        self.gs, self.shim, self.handle, self.count = gs, gs.shim, handle, count
        self.seed, self.first, self.stride, self.camera = seed, first, stride, camera

    @property
    def samples(self):
        """samples per pixel done so far"""
        return int(self.shim.rt_hip_accum_samples(self.handle))

    @property
    def kernel(self):
        """the member every pass runs (the plan made at creation)"""
        return self.shim.rt_hip_accum_kernel(self.handle).decode()

    def add(self, n, stats=None):
        """render the next n samples of every pixel; stats: an i64 [4] device tensor the pass's counters are added to"""
        dev = self.gs.dev
        _check(self.shim.rt_hip_accum_add(self.handle, n, stats.data_ptr() if stats is not None else None, _stream(dev)),
               "rt_hip_accum_add")
        return stats

    def resolve(self, tiles=None, tiles8=None):
        """the mean of the samples done -> (tiles f32 [count,64,3], tiles8 u8 [count,64,3]); pass buffers to reuse them"""
        dev = self.gs.dev
        if tiles is None:
            tiles = torch.empty((self.count, abi.TILE_PIXELS, 3), dtype=torch.float32, device=dev)
        if tiles8 is None:
            tiles8 = torch.empty((self.count, abi.TILE_PIXELS, 3), dtype=torch.uint8, device=dev)
        _check(self.shim.rt_hip_accum_resolve(self.handle, tiles.data_ptr(), tiles8.data_ptr(), _stream(dev)),
               "rt_hip_accum_resolve")
        return tiles, tiles8

    def denoised(self, **params):
        """The progressive preview: the mean of the samples done (resolve), the first-hit buffers of those samples, and the
        denoise (rt_hip_denoise; params: abi.denoise_params' keywords) -> (rgb f32 [H,W,3], rgb8 u8 [H,W,3]) on torch's current
        stream.  The accumulation must cover the whole image."""
        w, h = self.gs.scene.width, self.gs.scene.height
        total = n_tiles(w, h)
        if (self.first, self.stride, self.count) != (0, 1, total):
            raise ValueError("denoised(): the accumulation must cover the whole image (first 0, stride 1, every tile)")
        done = self.samples
        if done < 1:
            raise ValueError("denoised(): no samples done yet")
        tiles, tiles8 = self.resolve()
        image, _ = self.gs.untile(tiles, tiles8, 0, 1, total)
        aov = self.gs.untile_aov(self.gs.render_aov(self.seed, done, 0, 1, total, camera=self.camera, want=DENOISE_AOV), 0, 1, total)
        return denoise(image, aov, w, h, **params)

    @property
    def live_tiles(self):
        """how many slots still take samples (all of them until a freeze)"""
        return int(self.shim.rt_hip_accum_live_tiles(self.handle))

    def freeze(self, error=None, mask=None, threshold=None, dilate=None):
        """Stop tiles (rt_hip_accum_freeze): with `error` (an f32 [count] device tensor, tile_error's) every live slot whose own
        error and whose neighbours' within `dilate` tiles are <= threshold; with `mask` (one byte per slot, host or device, 0 =
        freeze) the slots the caller names.  Runs on torch's current stream and waits for the count -> live slots left."""
        if (error is None) == (mask is None):
            raise ValueError("freeze(): give the tile errors or a mask")
        dev = self.gs.dev
        live = C.c_uint32(0)
        if error is not None:
            p = abi.adapt_params(threshold=threshold, dilate=dilate)
            if not _is(error, dev, self.count, torch.float32):
                raise ValueError("freeze(): error must be a contiguous float32 tensor of one value per slot on the scene's device")
            _check(self.shim.rt_hip_accum_freeze(self.handle, _ptr(error), p.threshold, p.dilate, C.byref(live),
                                                 _stream(dev)), "rt_hip_accum_freeze")
        else:
            m = np.ascontiguousarray((mask.cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)) != 0, dtype=np.uint8)
            if m.size != self.count:
                raise ValueError("freeze(): mask must hold one value per slot")
            _check(self.shim.rt_hip_accum_freeze_mask(self.handle, C.c_void_p(m.ctypes.data), C.byref(live), _stream(dev)),
                   "rt_hip_accum_freeze_mask")
        return int(live.value)

    def tile_samples(self):
        """the sample-count map: numpy uint32 [count], how many samples each slot holds (synchronises)"""
        out = np.zeros(self.count, dtype=np.uint32)
        _check(self.shim.rt_hip_accum_tile_samples(self.handle, C.c_void_p(out.ctypes.data)), "rt_hip_accum_tile_samples")
        return out

    def run_adaptive(self, on_checkpoint=None, **params):
        """The adaptive driver (rt_hip_accum_run_adaptive; params: abi.adapt_params' keywords), synchronous on the null stream,
        from an empty accumulation.  on_checkpoint(samples_done, live_tiles) -> truthy to cancel.
        -> (stats dict of what was rendered, device seconds)"""
        p = abi.adapt_params(**params)
        stats = _host_counters()
        secs = C.c_double(0)
        cb = abi.ADAPT_CHECKPOINT(lambda user, done, live: 1 if on_checkpoint(done, live) else 0) if on_checkpoint else None
        _check(self.shim.rt_hip_accum_run_adaptive(self.handle, C.byref(p), stats, C.byref(secs),
                                                   C.cast(cb, C.c_void_p) if cb else None, None), "rt_hip_accum_run_adaptive")
        return _stats_dict(stats), secs.value

    def close(self):
        if self.handle:
            self.shim.rt_hip_accum_destroy(self.handle)
            self.handle.value = None   # the object GpuScene.close() holds too

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tile_error(cur, prev, width, height, first=0, stride=1, count=None, out=None):
    """rt_hip_tile_error on torch device tensors, asynchronous on torch's current stream: cur, prev f32 [count,64,3] compact tile
    buffers as Accumulation.resolve gives them (the means of the first n and of the first h < n samples) -> f32 [count], the
    error estimate of every slot"""
    dev = cur.device
    if count is None:
        count = n_tiles(width, height)
    if not all(_is(t, dev, count * abi.TILE_PIXELS * 3, torch.float32) for t in (cur, prev)):
        raise ValueError("tile_error(): cur and prev must be contiguous float32 tile buffers of count x 64 x 3 on one device")
    if out is None:
        out = torch.empty(count, dtype=torch.float32, device=dev)
    _check(abi.load_shim().rt_hip_tile_error(_ptr(cur), _ptr(prev), width, height, first, stride, count, _ptr(out), _stream(dev)),
           "rt_hip_tile_error")
    return out


DENOISE_AOV = ("albedo", "normal", "depth", "object", "hits")   # what the denoiser may read (object: OBJECT_EDGES only)


def denoise(rgb, aov, width, height, out=None, **params):
    """rt_hip_denoise on torch device tensors, asynchronous on torch's current stream: rgb f32 [H,W,3] (row-major, contiguous),
    aov a dict of row-major buffers as GpuScene.untile_aov gives them (normal, depth, hits; albedo with demodulate, object with
    object_edges), params abi.denoise_params' keywords.  out: an f32 [H,W,3] tensor for the result (it may be rgb itself).
    -> (rgb f32 [H,W,3], rgb8 u8 [H,W,3])"""
    dev = rgb.device
    shim = abi.load_shim()
    p = abi.denoise_params(**params)
    if not all(_is(t, dev) for t in [rgb] + list(aov.values())):
        raise ValueError("denoise(): every buffer must be a contiguous tensor on the colour's device")
    if rgb.dtype != torch.float32 or rgb.numel() != width * height * 3:
        raise ValueError("denoise(): rgb must be float32 of width * height * 3 values")

    def check(f, t):   # (of a feature buffer the count alone is asked, not the type)
        if t.numel() != width * height * abi.AOV_CHANNELS[f]:
            raise ValueError(f"denoise(): {f} must hold width * height * {abi.AOV_CHANNELS[f]} values")
    a = _aov_record(aov, [f for f in aov if f in abi.AOV_FIELDS], check)
    if out is None:
        out = torch.empty((height, width, 3), dtype=torch.float32, device=dev)
    elif not _is(out, dev, width * height * 3, torch.float32):
        raise ValueError("denoise(): out must be a contiguous float32 tensor of width * height * 3 values on the colour's device")
    out8 = torch.empty((height, width, 3), dtype=torch.uint8, device=dev)
    ws = torch.empty(max(shim.rt_hip_denoise_workspace_bytes(width, height), 1), dtype=torch.uint8, device=dev)
    _check(shim.rt_hip_denoise(_ptr(rgb), C.byref(a), width, height, C.byref(p), _ptr(ws), _ptr(out), _ptr(out8), _stream(dev)),
           "rt_hip_denoise")
    return out, out8


def _pixel_tensor(pixels, dev):
    """a list of pixel indices as a contiguous 32-bit tensor on `dev` (the uint32 words of the C-ABI)"""
    if isinstance(pixels, torch.Tensor):
        if pixels.element_size() != 4 or pixels.is_floating_point():
            raise ValueError("pixel indices must be a 32-bit integer tensor (the uint32 words of the C-ABI)")
        return pixels.to(dev).contiguous().reshape(-1)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(pixels, dtype=np.uint32).reshape(-1)).view(np.int32)).to(dev)


def select_pixels(values, w, h, lo, hi, invert=False, capacity=None, indices=None):
    """rt_hip_select_pixels on torch's current stream: values f32 of h x w (row-major, contiguous, on a device) -> (indices: an
    int32 tensor [capacity] holding the uint32 words p = y * w + x of the selected pixels, ascending, in its first min(count, capacity)
    entries -- the rest is left as it was --, count: how many pixels are selected; reading it back waits for the stream).
    capacity None: w * h; 0: count only (indices is None).  indices: a tensor to write into."""
    dev = values.device
    shim = abi.load_shim()
    if not _is(values, n=w * h, dtype=torch.float32):
        raise ValueError("select_pixels(): values must be a contiguous float32 tensor of w * h values")
    if capacity is None:
        capacity = indices.numel() if indices is not None else w * h
    if capacity and indices is None:
        indices = torch.empty(capacity, dtype=torch.int32, device=dev)
    if capacity and (not _is(indices, dev, size=4) or indices.numel() < capacity):
        raise ValueError("select_pixels(): indices must be a contiguous 32-bit tensor of at least `capacity` entries on the map's device")
    ws = torch.empty(max(shim.rt_hip_select_workspace_bytes(w, h), 1), dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    _check(shim.rt_hip_select_pixels(_ptr(values), w, h, lo, hi, abi.SELECT_INVERT if invert else 0, _ptr(ws),
                                     _ptr(indices) if capacity else None, capacity, _ptr(count), _stream(dev)), "rt_hip_select_pixels")
    return (indices if capacity else None), int(count.cpu().numpy().view("uint32")[0])


def blend_pixels(pixels, status, radiance, rgb, w, h, new_weight, prior_scale=0.0, prior=None, rgb8=None, weight=None, n=None):
    """rt_hip_blend_pixels on torch's current stream: the first n (None: all) entries of pixels (distinct 32-bit indices, as
    select_pixels gives them) with the status and radiance trace_pixels gave for them go into rgb (f32 of h x w x 3, in place):
    replaced where prior_scale * prior is not positive and finite, else blended with weight new_weight against it.  prior: f32 of
    h x w (None: 1.0); rgb8 (u8 of h x w x 3) and weight (f32 of h x w; it may be prior itself) are written at the touched pixels."""
    dev = rgb.device
    pixels = _pixel_tensor(pixels, dev)
    n = pixels.numel() if n is None else int(n)
    if n < 0 or n > pixels.numel() or status.numel() < n or radiance.numel() < 3 * n:
        raise ValueError("blend_pixels(): n must be within the list, its status and its radiance")
    if not _is(status, dev, size=4) or not _is(radiance, dev, dtype=torch.float64):
        raise ValueError("blend_pixels(): status (32-bit) and radiance (float64) must be contiguous tensors on the frame's device")
    if not _is(rgb, n=w * h * 3, dtype=torch.float32):
        raise ValueError("blend_pixels(): rgb must be a contiguous float32 tensor of w * h * 3 values")
    for t, dtype, k, what in ((prior, torch.float32, 1, "prior"), (weight, torch.float32, 1, "weight"), (rgb8, torch.uint8, 3, "rgb8")):
        if t is not None and not _is(t, dev, w * h * k, dtype):
            raise ValueError(f"blend_pixels(): {what} must be a contiguous {dtype} tensor of w * h * {k} values on the frame's device")
    lists = [_ptr(t) if n else None for t in (pixels, status, radiance)]   # (no entry: no list)
    _check(abi.load_shim().rt_hip_blend_pixels(*lists, n, w, h, new_weight, prior_scale, _ptr(prior), _ptr(rgb), _ptr(rgb8), _ptr(weight),
                                               _stream(dev)), "rt_hip_blend_pixels")
    return rgb


def trace_pixels_host(scene, pixels, samples, seed, sample_first=0, camera=None, max_depth=None, device=0, want=("status", "radiance")):
    """rt_hip_trace_pixels_host(): the C hosts' entry point (its own scene and buffers on logical device `device`, synchronous) ->
    dict of numpy arrays: status uint32 [n], radiance float64 [n, 3], samples [n, samples, 3], paths / casts uint64 [n], and stats"""
    shim = abi.load_shim()
    pixels = np.ascontiguousarray(np.asarray(pixels, dtype=np.uint32).reshape(-1))
    n = pixels.size
    p = abi.pixel_params(scene.width, scene.height, samples, seed, sample_first, _depth(scene, max_depth))
    out, rad = _wanted(abi.RtHipRadiance(), abi.RADIANCE_SHAPES, want, n, None, samples)
    stats = _host_counters()
    _check(shim.rt_hip_trace_pixels_host(*_host_scene(scene), C.byref(_camera(scene, camera)), pixels.ctypes.data, n, C.byref(p), device,
                                         C.byref(rad), stats), "rt_hip_trace_pixels_host")
    out["stats"] = _stats_dict(stats)
    return out


REPROJECT_AOV = ("normal", "depth", "object", "hits")   # what rt_hip_reproject reads of a frame and of the history


def _frame_aov(name, aov, fields, n, dev, what, needed=False):
    """The RtHipAov of a frame's row-major device buffers for reproject() / upsample(): each of `fields` a contiguous tensor of 4-byte
    elements and n pixels on dev.  needed: a missing field is refused by name (else it is a KeyError)."""
    def check(f, t):
        if needed and f not in aov:
            raise ValueError(f"{name}(): {what} {f} buffer is needed")
        if not _is(t, dev, n * abi.AOV_CHANNELS[f], size=4):
            raise ValueError(f"{name}(): {what} {f} must be a contiguous 32-bit tensor of width * height * {abi.AOV_CHANNELS[f]} "
                             "values on the colour's device")
    return _aov_record(aov, fields, check, optional=needed)


def _reproject_aov(aov, n, dev, what):
    return _frame_aov("reproject", aov, REPROJECT_AOV, n, dev, what)


def _upsample_aov(aov, n, dev, p, what):
    need = ["normal", "depth", "hits"] + (["albedo"] if p.flags & abi.UPSAMPLE_DEMODULATE else []) + \
           (["object"] if p.flags & abi.UPSAMPLE_OBJECT_EDGES else [])
    return _frame_aov("upsample", aov, need, n, dev, what, needed=True)


def _out_dict(name, out, shapes, dev):
    """The one rule of an `out` dict, shapes: {field: (shape, dtype, optional)} -> the filled dict: what is missing is allocated, an
    optional field given as None is not wanted and leaves the dict, what is given is checked."""
    out = dict(out) if out else {}
    for f, (shape, dtype, optional) in shapes.items():
        if optional and f in out and out[f] is None:
            del out[f]
            continue
        if f not in out:
            out[f] = torch.empty(shape, dtype=dtype, device=dev)
        if not _is(out[f], dev, math.prod(shape), dtype):
            raise ValueError(f"{name}(): out[{f!r}] must be a contiguous {dtype} tensor of shape {shape} on the colour's device")
    return out


def _sphere_pair(name, spheres_prev, spheres_cur, check):
    """(n_spheres, prev, cur) of the two sphere arrays of prev_points_moved*(): both None, or both float64 (n, 4)"""
    if spheres_prev is None and spheres_cur is None:
        return 0, None, None
    if spheres_prev is None or spheres_cur is None:
        raise ValueError(f"{name}(): spheres_prev and spheres_cur go together")
    prev, cur = check(spheres_prev), check(spheres_cur)
    if prev.shape != cur.shape:
        raise ValueError(f"{name}(): spheres_prev and spheres_cur must have the same shape")
    return int(prev.shape[0]), prev, cur


def _prev_points(name, hits, positions, spheres=None, out=None, device=None):
    """The one body of prev_points(), prev_points_moved() and their host forms.  spheres: None (rt_hip_prev_points*) or the pair
    (spheres_prev, spheres_cur) (rt_hip_prev_points_moved*, which reads hits["object"] too).  device None: torch tensors on the hits'
    device, on torch's current stream; else numpy arrays and the host form on that logical device.  An array of no entries goes down
    as the address 1: nothing reads it, it only says "given"."""
    host = device is not None
    address = (lambda a, some=True: a.ctypes.data if some else 1) if host else (lambda t, some=True: C.c_void_p(t.data_ptr() if some else 1))
    h, dev, n = abi.RtHipHits(), None, None
    h.kept = []   # (what a host form converted stays alive with the record)
    for f in ("status", "prim", "bary", "point") if spheres is None else ("status", "prim", "object", "bary", "point"):
        dtype, k = abi.HIT_SHAPES[f]
        t = np.ascontiguousarray(hits[f], dtype=dtype) if host else hits[f]
        if n is None:   # (status: it says how many)
            dev, n = (None, t.size) if host else (t.device, int(t.numel()))
        if host and t.size != n * k:
            raise ValueError(f"{name}(): hits[{f!r}] must hold {n} x {k} values")
        if not host and not _is(t, dev, n * k, _TORCH[dtype]):
            raise ValueError(f"{name}(): hits[{f!r}] must be a contiguous tensor of {n} x {k} values as a query returns it")
        h.kept.append(t)
        setattr(h, f, (t.ctypes.data if host else t.data_ptr()) if n else 1)
    pos = None
    if positions is not None and host:
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3, 3)
    elif positions is not None:
        if positions.dtype != torch.float64 or positions.dim() != 3 or tuple(positions.shape[1:]) != (3, 3) or positions.device != dev:
            raise ValueError(f"{name}(): positions must be a float64 tensor of shape (n_triangles, 3, 3) on the hits' device")
        pos = positions.contiguous()
    n_tri = 0 if pos is None else int(pos.shape[0])
    moved = ()
    if spheres is not None:
        def check(t):
            if host:
                return np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 4)
            if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 4 or t.device != dev:
                raise ValueError(f"{name}(): the spheres must be float64 tensors of shape (n_spheres, 4) on the hits' device")
            return t.contiguous()
        n_sph, sprev, scur = _sphere_pair(name, *spheres, check)
        # (an empty pair is still "given": a sphere hit then has no sphere to ride, NaN)
        moved = tuple(None if a is None else address(a, n_sph) for a in (sprev, scur)) + (n_sph,)
    if host:
        out = np.zeros((n, 3), np.float64)
    elif out is None:
        out = torch.empty((n, 3), dtype=torch.float64, device=dev)
    elif not _is(out, dev, 3 * n, torch.float64):
        raise ValueError(f"{name}(): out must be a contiguous float64 tensor of {n} x 3 values on the hits' device")
    symbol = "rt_hip_" + name
    _check(getattr(abi.load_shim(), symbol)(C.byref(h), n, address(pos) if n_tri else None, n_tri, *moved,
                                            *((device, address(out, n)) if host else (address(out, n), _stream(dev)))), symbol)
    return out


def prev_points(hits, positions, out=None):
    """rt_hip_prev_points on torch device tensors, asynchronous on torch's current stream: where each hit point of a query was
    before an update_vertices.  hits: a dict as GpuScene.query_rays / query_uv return it, with status, prim, bary and point;
    positions: float64 (n_triangles, 3, 3), the positions the scene had at the previous frame, in update_vertices' layout (None:
    no triangles); out: float64 [n, 3] to write into (it may be hits["point"]; None: allocated) -> float64 [n, 3], NaN where there
    is no surface to follow (a miss, an invalid ray, a prim outside the positions)"""
    return _prev_points("prev_points", hits, positions, out=out)


def prev_points_moved(hits, positions, spheres_prev, spheres_cur, out=None):
    """rt_hip_prev_points_moved on torch device tensors, asynchronous on torch's current stream: prev_points() across an
    update_spheres as well.  hits needs object too; spheres_prev / spheres_cur: float64 (n_spheres, 4), cx cy cz radius in object
    order, the spheres at the previous frame and now (both None: no sphere moved, prev_points() itself).  A hit on a sphere rides
    its translation and uniform scale; a sphere hit whose object is outside the arrays gives NaN."""
    return _prev_points("prev_points_moved", hits, positions, (spheres_prev, spheres_cur), out)


def prev_points_moved_host(hits, positions, spheres_prev, spheres_cur, device=0):
    """rt_hip_prev_points_moved_host(): host arrays, its own device buffers on logical device `device`, synchronous.  hits: numpy
    arrays with status, prim, object (uint32 [n]), bary (float64 [n, 2]) and point (float64 [n, 3]); positions: float64
    (n_triangles, 3, 3) or None; spheres_prev / spheres_cur: float64 (n_spheres, 4) or both None -> float64 [n, 3]"""
    return _prev_points("prev_points_moved_host", hits, positions, (spheres_prev, spheres_cur), device=device)


def prev_points_host(hits, positions, device=0):
    """rt_hip_prev_points_host(): host arrays, its own device buffers on logical device `device`, synchronous.  hits: a dict of
    numpy arrays with status, prim (uint32 [n]), bary (float64 [n, 2]) and point (float64 [n, 3]); positions: float64
    (n_triangles, 3, 3) or None -> float64 [n, 3]"""
    return _prev_points("prev_points_host", hits, positions, device=device)


def reproject(rgb, aov, camera, hist=None, out=None, prev_points=None, **params):
    """rt_hip_reproject on torch device tensors, asynchronous on torch's current stream: rgb f32 [H,W,3] (row-major, contiguous),
    aov a dict of row-major buffers as GpuScene.untile_aov gives them (normal, depth, object, hits), camera the frame's abi.Camera.
    hist: None (the first frame) or a dict with rgb and len (an earlier call's results), aov and camera (that frame's).  out: a
    dict of tensors to write into (rgb f32 [H,W,3] -- it may be the input rgb --, len f32 [H,W], motion f32 [H,W,2], rgb8 u8
    [H,W,3]; what is missing is allocated; motion or rgb8 given as None: not wanted, not computed), none of them a history buffer
    or another buffer of the call.  params: abi.reproject_params' keywords.
    prev_points (None: the scene is static between the two frames, rt_hip_reproject): float64 [H,W,3], where each pixel's
    surface point was in the history's frame, as prev_points() gives it for the pixel-centre query -- the reprojection starts
    from it instead of the depth along the frame's ray (rt_hip_reproject_points), and a pixel whose point is not finite starts
    a new history.
    -> dict(rgb, len, and motion and rgb8 unless not wanted)"""
    dev = rgb.device
    shim = abi.load_shim()
    p = abi.reproject_params(**params)
    if rgb.dim() != 3 or rgb.shape[2] != 3 or rgb.dtype != torch.float32 or not rgb.is_contiguous():
        raise ValueError("reproject(): rgb must be a contiguous float32 [H,W,3] tensor")
    height, width = int(rgb.shape[0]), int(rgb.shape[1])
    n = width * height
    a = _reproject_aov(aov, n, dev, "the frame's")
    h_rgb = h_len = h_aov = h_cam = None
    if hist is not None:
        for f in ("rgb", "len"):
            if not _is(hist[f], dev, n * (3 if f == "rgb" else 1), torch.float32):
                raise ValueError(f"reproject(): the history's {f} must be a contiguous float32 tensor of the frame's size on its device")
        h_rgb, h_len = _ptr(hist["rgb"]), _ptr(hist["len"])
        h_aov, h_cam = C.byref(_reproject_aov(hist["aov"], n, dev, "the history's")), C.byref(hist["camera"])
    out = _out_dict("reproject", out, dict(rgb=((height, width, 3), torch.float32, False), len=((height, width), torch.float32, False),
                                           motion=((height, width, 2), torch.float32, True), rgb8=((height, width, 3), torch.uint8, True)), dev)
    frames = (_ptr(rgb), C.byref(a), C.byref(camera), h_rgb, h_len, h_aov, h_cam, width, height, C.byref(p))
    outs = (_ptr(out["rgb"]), _ptr(out.get("rgb8")), _ptr(out["len"]), _ptr(out.get("motion")), _stream(dev))
    if prev_points is None:
        _check(shim.rt_hip_reproject(*frames, *outs), "rt_hip_reproject")
        return out
    if not _is(prev_points, dev, 3 * n, torch.float64):
        raise ValueError("reproject(): prev_points must be a contiguous float64 tensor of width * height * 3 values on the colour's device")
    _check(shim.rt_hip_reproject_points(*frames, _ptr(prev_points), *outs), "rt_hip_reproject_points")
    return out


class Temporal:
    """Frames of one scene under a moving camera (GpuScene.temporal): every frame is rendered, its first-hit buffers of the same
    samples are rendered, and it is accumulated onto the history of the frames before it where the reprojection finds the same
    surface (rt_hip.h, rt_hip_reproject).  The history -- accumulated colour, length, the first-hit buffers and the camera -- is
    double-buffered and allocated once; frame() runs on torch's current stream.  The scene must stay open; its triangles may
    move between frames (GpuScene.update_vertices) when frame() is given the positions they had at the previous frame."""

    def __init__(self, gs, **params):
        self.gs = gs
        self.params = params
        abi.reproject_params(**params)   # a bad keyword fails here
        w, h = gs.scene.width, gs.scene.height
        dev = gs.dev
        self._total = n_tiles(w, h)

        def slot():
            aov = dict(normal=torch.zeros((h, w, 3), dtype=torch.float32, device=dev), depth=torch.zeros((h, w), dtype=torch.float32, device=dev),
                       object=torch.zeros((h, w), dtype=torch.int32, device=dev), hits=torch.zeros((h, w), dtype=torch.int32, device=dev),
                       albedo=torch.zeros((h, w, 3), dtype=torch.float32, device=dev))
            return dict(rgb=torch.zeros((h, w, 3), dtype=torch.float32, device=dev), len=torch.zeros((h, w), dtype=torch.float32, device=dev),
                        aov=aov, camera=abi.Camera())
        self._slots = [slot(), slot()]
        self._tiles = torch.empty((self._total, abi.TILE_PIXELS, 3), dtype=torch.float32, device=dev)
        self._tiles8 = torch.empty((self._total, abi.TILE_PIXELS, 3), dtype=torch.uint8, device=dev)
        self._motion = torch.zeros((h, w, 2), dtype=torch.float32, device=dev)
        self._rgb8 = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
        # frames across update_vertices (prev_positions): the pixel-centre grid of rt_hip_reproject's step 3, the query's hit
        # buffers and the previous points
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
        self._uv = torch.stack([(xs + 0.5) / (float(w) - 1.0), (ys + 0.5) / (float(h) - 1.0)], dim=-1).reshape(-1, 2).contiguous().to(dev)
        self._hits = dict(status=torch.zeros(w * h, dtype=torch.int32, device=dev), prim=torch.zeros(w * h, dtype=torch.int32, device=dev),
                          bary=torch.zeros((w * h, 2), dtype=torch.float64, device=dev), point=torch.zeros((w * h, 3), dtype=torch.float64, device=dev),
                          object=torch.zeros(w * h, dtype=torch.int32, device=dev))
        self._points = torch.zeros((w * h, 3), dtype=torch.float64, device=dev)
        self._cur = 0          # the slot the next frame is written to
        self.frames = 0        # frames since the last reset: 0 = the next one has no history

    def _denoised(self, slot, **denoise_params):
        return denoise(slot["rgb"], slot["aov"], self.gs.scene.width, self.gs.scene.height, **denoise_params)

    def reset(self):
        """drop the history: the next frame starts from its own samples"""
        self.frames = 0

    def frame(self, camera, seed, samples, max_depth=None, denoise=False, fill=None, prev_positions=None, prev_spheres=None,
              **denoise_params):
        """Render `samples` per pixel under `camera` (an abi.Camera), reproject and accumulate -> dict of device tensors, valid
        until the next frame(): rgb f32 [H,W,3] (the accumulated image), rgb8 u8 [H,W,3], len f32 [H,W], motion f32
        [H,W,2], aov (the frame's first-hit buffers), and with denoise: denoised / denoised8, rt_hip_denoise of the accumulated
        image under the frame's buffers (denoise_params: abi.denoise_params' keywords).
        fill (None: nothing, the frame is what it was without the argument; or S >= 1): after the reprojection the pixels with
        0 <= len <= 1 -- disoccluded, or not to be used -- get S more samples of the render's own, from sample `samples` on
        (GpuScene.refine with prior = len, prior_scale = samples: a pixel of length 1 blends its `samples` samples with the S new
        ones, a pixel of length 0 is replaced), and their len becomes (len * samples + S) / samples, rounded as rt_hip_blend_pixels'
        weight and then divided in float32; res["filled"] is how many (the call then waits for that one word).
        prev_positions (None: the scene has not moved since the previous frame()): the float64 (n_triangles, 3, 3) device tensor
        of the positions the scene had at the previous frame(), after an update_vertices.  With a history, the pixel centres are
        queried under `camera` (query_uv), each hit is taken back to those positions (prev_points) and the reprojection starts
        from there (reproject(prev_points=...)): the history follows the moving surface.
        prev_spheres (None: no sphere has moved since the previous frame()): the float64 (n_objects, 4) device tensor of the
        spheres the scene had at the previous frame(), after an update_spheres -- the sphere twin of prev_positions.  With either,
        the same query feeds prev_points_moved with the scene's current spheres (GpuScene.spheres())."""
        gs, total = self.gs, self._total
        w, h = gs.scene.width, gs.scene.height
        cur, prev = self._slots[self._cur], self._slots[self._cur ^ 1]
        chunks = gs.suggest_chunks(total, samples, max_depth)
        tiles, _, _ = gs.render_tiles(seed, 0, 1, total, tiles=self._tiles, tiles8=self._tiles8, samples=samples, max_depth=max_depth,
                                      chunks=chunks, camera=camera)
        gs.untile(tiles, None, 0, 1, total, image=cur["rgb"])
        at = gs.render_aov(seed, samples, 0, 1, total, camera=camera, want=DENOISE_AOV)
        gs._untile_aov(at, 0, 1, total, cur["aov"])
        C.memmove(C.byref(cur["camera"]), C.byref(camera), C.sizeof(abi.Camera))
        points = None
        if (prev_positions is not None or prev_spheres is not None) and self.frames:
            hits = gs.query_uv(self._uv, camera=camera, want=("status", "prim", "object", "bary", "point"), out=self._hits)
            # (without prev_spheres this is prev_points' own arithmetic: a sphere hit keeps its point, bit for bit)
            points = prev_points_moved(hits, prev_positions, prev_spheres, None if prev_spheres is None else gs.spheres(), out=self._points)
        res = reproject(cur["rgb"], cur["aov"], cur["camera"], hist=prev if self.frames else None,
                        out=dict(rgb=cur["rgb"], len=cur["len"], motion=self._motion, rgb8=self._rgb8), prev_points=points, **self.params)
        res["aov"] = cur["aov"]
        if fill is not None:
            if int(fill) != fill or fill < 1:
                raise ValueError("frame(): fill must be an integer >= 1")
            weight = torch.zeros((h, w), dtype=torch.float32, device=cur["len"].device)
            idx, count = select_pixels(cur["len"], w, h, 0.0, 1.0)
            if count:
                out = gs.trace_pixels(idx, int(fill), seed, sample_first=samples, camera=camera, max_depth=max_depth, n=count)
                blend_pixels(idx, out["status"], out["radiance"], cur["rgb"], w, h, float(fill), float(samples), prior=cur["len"],
                             rgb8=self._rgb8, weight=weight, n=count)
                at = idx[:count].long()   # (plumbing: the weights, in samples, back into the length map, in frames)
                got, flat = weight.view(-1)[at], cur["len"].view(-1)
                flat[at] = torch.where(got > 0, got / float(samples), flat[at])   # (weight 0: the blend left the pixel untouched)
            res["filled"] = count
        if denoise:
            res["denoised"], res["denoised8"] = self._denoised(cur, **denoise_params)
        self._cur ^= 1
        self.frames += 1
        return res


def reproject_image_host(rgb, aov, camera, hist=None, device=0, prev_points=None, **params):
    """rt_hip_reproject_image(): the C hosts' entry point (host arrays, its own device buffers on logical device `device`,
    synchronous).  rgb float32 [H,W,3], aov a dict of numpy arrays as GpuScene.aov_image gives them, hist None or a dict with rgb,
    len, aov and camera; prev_points: None, or float64 [H,W,3] (rt_hip_reproject_points_image) -> dict of numpy arrays: rgb,
    rgb8, len, motion"""
    shim = abi.load_shim()
    p = abi.reproject_params(**params)
    h, w = rgb.shape[:2]
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    a = _aov_record(aov, REPROJECT_AOV, host=True)
    h_rgb = h_len = h_aov = h_cam = None
    if hist is not None:
        hr, hl = np.ascontiguousarray(hist["rgb"], dtype=np.float32), np.ascontiguousarray(hist["len"], dtype=np.float32)
        h_rgb, h_len = hr.ctypes.data, hl.ctypes.data
        h_aov, h_cam = C.byref(_aov_record(hist["aov"], REPROJECT_AOV, host=True)), C.byref(hist["camera"])
    out = dict(rgb=np.zeros((h, w, 3), np.float32), rgb8=np.zeros((h, w, 3), np.uint8), len=np.zeros((h, w), np.float32),
               motion=np.zeros((h, w, 2), np.float32))
    frames = (rgb.ctypes.data, C.byref(a), C.byref(camera), h_rgb, h_len, h_aov, h_cam, w, h, C.byref(p))
    outs = (out["rgb"].ctypes.data, out["rgb8"].ctypes.data, out["len"].ctypes.data, out["motion"].ctypes.data)
    if prev_points is None:
        _check(shim.rt_hip_reproject_image(*frames, device, *outs), "rt_hip_reproject_image")
        return out
    pts = np.ascontiguousarray(prev_points, dtype=np.float64)
    if pts.size != 3 * w * h:
        raise ValueError("reproject_image_host(): prev_points must hold width * height * 3 values")
    _check(shim.rt_hip_reproject_points_image(*frames, pts.ctypes.data, device, *outs), "rt_hip_reproject_points_image")
    return out


UPSAMPLE_AOV = ("albedo", "normal", "depth", "object", "hits")   # what rt_hip_upsample may read (albedo, object: by the flags)


def upsample(low_rgb, low_aov, wl, hl, aov, w, h, out=None, **params):
    """rt_hip_upsample on torch device tensors, asynchronous on torch's current stream: low_rgb f32 of hl x wl x 3 values (row-major,
    contiguous), low_aov and aov dicts of row-major buffers as GpuScene.untile_aov gives them at wl x hl and at w x h (normal,
    depth, hits; albedo with demodulate, object with object_edges).  out: a dict of tensors to write into (rgb f32 [h,w,3], rgb8 u8
    [h,w,3], conf f32 [h,w]; what is missing is allocated; rgb8 or conf given as None: not wanted, not computed), none of them a
    buffer the call reads.  params: abi.upsample_params' keywords.  -> dict(rgb, and rgb8 and conf unless not wanted)"""
    dev = low_rgb.device
    shim = abi.load_shim()
    p = abi.upsample_params(**params)
    if not _is(low_rgb, n=wl * hl * 3, dtype=torch.float32):
        raise ValueError("upsample(): low_rgb must be a contiguous float32 tensor of wl * hl * 3 values")
    la, a = _upsample_aov(low_aov, wl * hl, dev, p, "the low frame's"), _upsample_aov(aov, w * h, dev, p, "the full frame's")
    out = _out_dict("upsample", out, dict(rgb=((h, w, 3), torch.float32, False), rgb8=((h, w, 3), torch.uint8, True),
                                          conf=((h, w), torch.float32, True)), dev)
    _check(shim.rt_hip_upsample(_ptr(low_rgb), C.byref(la), wl, hl, C.byref(a), w, h, C.byref(p), _ptr(out["rgb"]), _ptr(out.get("rgb8")),
                                _ptr(out.get("conf")), _stream(dev)), "rt_hip_upsample")
    return out


class Preview:
    """Frames of one scene at a fraction of the pixels (GpuScene.preview): the colour is rendered -- and, if wanted, denoised -- at
    ceil(width / scale) x ceil(height / scale) by a second GpuScene of that size under the FULL frame's camera (get_camera_ray's
    (x + r) / (w - 1) ties the two pixel grids together), the first-hit buffers are rendered at both sizes, and rt_hip_upsample
    brings the colour to full size under the full-resolution ones.  frame() runs on torch's current stream.  The scene must stay
    open and unchanged; close() frees the low scene."""

    def __init__(self, gs, scale, **params):
        import dataclasses
        if int(scale) != scale or scale < 2:
            raise ValueError("preview(): scale must be an integer >= 2")
        self.gs, self.scale, self.params = gs, int(scale), params
        abi.upsample_params(**params)   # a bad keyword fails here
        sc = gs.scene
        self.low_width, self.low_height = -(-sc.width // self.scale), -(-sc.height // self.scale)
        if self.low_width < 2 or self.low_height < 2:
            raise ValueError(f"preview(): the low frame would be {self.low_width} x {self.low_height}; both sides must be at least 2")
        # the same objects, meshes and camera bytes at another size: nothing is rebuilt (a room's walls follow the FULL aspect)
        self.low = GpuScene(dataclasses.replace(sc, width=self.low_width, height=self.low_height), device=gs.device)

    def close(self):
        self.low.close()

    def _denoised(self, rgb, aov, **denoise_params):
        return denoise(rgb, aov, self.low_width, self.low_height, **denoise_params)

    def frame(self, seed, samples, camera=None, denoise=False, fill=None, **denoise_params):
        """Render `samples` per pixel at the low size under `camera` (an abi.Camera; None: the scene's own), the first-hit buffers
        of `samples` camera samples at both sizes, and upsample -> dict of device tensors: rgb f32 [H,W,3], rgb8 u8 [H,W,3], conf
        f32 [H,W] (rt_hip.h: 1 .. 0 guided, 0 plain bilinear, -1 nothing usable), aov (the full-size buffers) and low (dict: rgb
        -- denoised with denoise=True, by rt_hip_denoise under the low buffers with denoise_params, abi.denoise_params' keywords --,
        noisy: the low frame as rendered, aov).
        fill (None: nothing, the frame is what it was without the argument; or S >= 1): after the upsampling the pixels with
        conf <= 0 -- plain bilinear, or nothing -- are REPLACED by the mean of the full-size render's own samples 0 .. S - 1 of them
        (GpuScene.refine, prior_scale 0), floats and bytes; res["filled"] is how many (the call then waits for that one word)."""
        gs, lo = self.gs, self.low
        w, h, wl, hl = gs.scene.width, gs.scene.height, self.low_width, self.low_height
        total, total_low = n_tiles(w, h), n_tiles(wl, hl)
        tiles, _, _ = lo.render_tiles(seed, 0, 1, total_low, samples=samples, chunks=lo.suggest_chunks(total_low, samples), camera=camera)
        noisy, _ = lo.untile(tiles, None, 0, 1, total_low)
        low_aov = lo.untile_aov(lo.render_aov(seed, samples, 0, 1, total_low, camera=camera, want=UPSAMPLE_AOV), 0, 1, total_low)
        rgb = noisy
        if denoise:
            rgb, _ = self._denoised(noisy, low_aov, **denoise_params)
        aov = gs.untile_aov(gs.render_aov(seed, samples, 0, 1, total, camera=camera, want=UPSAMPLE_AOV), 0, 1, total)
        res = upsample(rgb, low_aov, wl, hl, aov, w, h, **self.params)
        res.update(aov=aov, low=dict(rgb=rgb, noisy=noisy, aov=low_aov))
        if fill is not None:
            if int(fill) != fill or fill < 1:
                raise ValueError("frame(): fill must be an integer >= 1")
            if "conf" not in res:
                raise ValueError("frame(): fill needs the confidence map")
            res["filled"] = gs.refine(res["rgb"], res["conf"], float("-inf"), 0.0, int(fill), seed, sample_first=0, camera=camera,
                                      rgb8=res.get("rgb8"))
        return res


def upsample_image_host(low_rgb, low_aov, aov, device=0, **params):
    """rt_hip_upsample_image(): the C hosts' entry point (host arrays, its own device buffers on logical device `device`,
    synchronous).  low_rgb float32 [hl,wl,3], low_aov and aov dicts of numpy arrays as GpuScene.aov_image gives them at the two
    sizes -> dict of numpy arrays: rgb, rgb8, conf"""
    shim = abi.load_shim()
    p = abi.upsample_params(**params)
    la, a = (_aov_record(bufs, UPSAMPLE_AOV, optional=True, host=True) for bufs in (low_aov, aov))
    low_rgb = np.ascontiguousarray(low_rgb, dtype=np.float32)
    hl, wl = low_rgb.shape[:2]
    h, w = np.asarray(aov["depth"]).shape
    out = dict(rgb=np.zeros((h, w, 3), np.float32), rgb8=np.zeros((h, w, 3), np.uint8), conf=np.zeros((h, w), np.float32))
    _check(shim.rt_hip_upsample_image(low_rgb.ctypes.data, C.byref(la), wl, hl, C.byref(a), w, h, C.byref(p), device,
                                      out["rgb"].ctypes.data, out["rgb8"].ctypes.data, out["conf"].ctypes.data), "rt_hip_upsample_image")
    return out


def render_image_host(scene, seed, n_devices=1, samples=None, max_depth=None, integrator="path"):
    """rt_hip_render_image(): the C hosts' entry point (host buffers, synchronous)."""
    shim = abi.load_shim()
    p = _params(scene, seed, samples or scene.samples, _depth(scene, max_depth), integrator)
    img, img8 = _frame_pair(scene.height, scene.width, None)
    stats = _host_counters()
    secs = C.c_double(0)
    _check(shim.rt_hip_render_image(*_host_scene(scene), C.byref(scene.camera), C.byref(p), n_devices, img.ctypes.data, img8.ctypes.data, stats,
                                    C.byref(secs)), "rt_hip_render_image")
    return img, img8, _stats_dict(stats), secs.value


def aov_image_host(scene, seed, samples, device=0):
    """rt_hip_render_aov_image(): the C hosts' entry point (its own scene on logical device `device`, synchronous) -> dict of
    row-major numpy arrays as GpuScene.aov_image"""
    shim = abi.load_shim()
    p = _params(scene, seed, samples, 0)   # (first hits: no depth to give)
    h, w = scene.height, scene.width
    out = {f: np.zeros(_aov_shape(f, h, w), dtype=abi.AOV_DTYPES[f]) for f in abi.AOV_FIELDS}
    _check(shim.rt_hip_render_aov_image(*_host_scene(scene), C.byref(scene.camera), C.byref(p), device, C.byref(_aov_record(out, abi.AOV_FIELDS, host=True))), "rt_hip_render_aov_image")
    return out


def adaptive_image_host(scene, seed, samples, device=0, max_depth=None, integrator="path", **params):
    """rt_hip_render_adaptive_image(): the C hosts' entry point (its own scene and accumulation on logical device `device`,
    synchronous; params: abi.adapt_params' keywords) -> (image f32 [H,W,3], image8 u8 [H,W,3], tile sample counts uint32
    [tiles_y, tiles_x], stats dict, device seconds)"""
    shim = abi.load_shim()
    p = _params(scene, seed, samples, _depth(scene, max_depth), integrator)
    ap = abi.adapt_params(**params)
    h, w = scene.height, scene.width
    img, img8 = _frame_pair(h, w, None)
    counts = np.zeros(((h + abi.TILE - 1) // abi.TILE, (w + abi.TILE - 1) // abi.TILE), np.uint32)
    stats = _host_counters()
    secs = C.c_double(0)
    _check(shim.rt_hip_render_adaptive_image(*_host_scene(scene), C.byref(scene.camera), C.byref(p), C.byref(ap), device, img.ctypes.data,
                                             img8.ctypes.data, counts.ctypes.data, stats, C.byref(secs), None, None),
           "rt_hip_render_adaptive_image")
    return img, img8, counts, _stats_dict(stats), secs.value


def _host_rays(rays, camera):
    """(rays, n, source) of a host query: float64 [n, 6] given rays, or with a camera [n, 2] (u, v)"""
    rays = np.ascontiguousarray(np.asarray(rays, dtype=np.float64).reshape(-1, 2 if camera is not None else 6))
    return rays, rays.shape[0], abi.RAYS_CAMERA_UV if camera is not None else abi.RAYS_GIVEN


def query_rays_host(scene, rays, t_max=None, normalize=False, origin_radius=None, camera=None, device=0, want=abi.HIT_FIELDS):
    """rt_hip_query_rays_host(): the C hosts' entry point (its own scene and buffers on logical device `device`, synchronous).
    rays: [n, 6] float64 (origin, direction), or with `camera` (an abi.Camera) [n, 2] (u, v) -> dict of numpy arrays: status /
    object / prim uint32 [n], t float64 [n], point / normal [n, 3], bary [n, 2], ray [n, 6]"""
    shim = abi.load_shim()
    rays, n, source = _host_rays(rays, camera)
    if t_max is not None:
        t_max = np.ascontiguousarray(np.asarray(t_max, dtype=np.float64).reshape(-1))
        if t_max.size != n:
            raise ValueError("query_rays_host: t_max must hold one value per ray")
    p = abi.query_params(source, normalize, camera, origin_radius)
    out, hits = _wanted(abi.RtHipHits(), abi.HIT_SHAPES, want, n, None)
    _check(shim.rt_hip_query_rays_host(*_host_scene(scene), rays.ctypes.data,
                                       t_max.ctypes.data if t_max is not None else None, n, C.byref(p), device, C.byref(hits)),
           "rt_hip_query_rays_host")
    return out


def trace_rays_host(scene, rays, samples, seed, max_depth=None, normalize=False, origin_radius=None, camera=None, index_first=0,
                    device=0, want=("status", "radiance")):
    """rt_hip_trace_rays_host(): the C hosts' entry point (its own scene and buffers on logical device `device`, synchronous).
    rays: [n, 6] float64 (origin, direction), or with `camera` (an abi.Camera) [n, 2] (u, v) -> dict of numpy arrays: status uint32
    [n], radiance float64 [n, 3], samples [n, samples, 3], paths / casts uint64 [n], ray [n, 6], and stats (a dict)"""
    shim = abi.load_shim()
    rays, n, source = _host_rays(rays, camera)
    p = abi.trace_params(samples, seed, _depth(scene, max_depth), source, normalize, camera, origin_radius, index_first)
    out, rad = _wanted(abi.RtHipRadiance(), abi.RADIANCE_SHAPES, want, n, None, samples)
    stats = _host_counters()
    _check(shim.rt_hip_trace_rays_host(*_host_scene(scene), rays.ctypes.data, n, C.byref(p), device, C.byref(rad), stats),
           "rt_hip_trace_rays_host")
    out["stats"] = _stats_dict(stats)
    return out


def lens_rays(camera, width, height, aperture, focus, seed, sample, pixel_first=0, n=None, device=0):
    """The lens rays of one sample pass (rt_hip.h, rt_hip_lens_rays): pixels [pixel_first, pixel_first + n) (n None: to the frame's
    end) of sample `sample` -> a device tensor [n, 6] float64 (origin, direction), asynchronous on torch's current stream"""
    shim = abi.load_shim()
    dev = torch.device("cuda", device)
    n = width * height - pixel_first if n is None else n
    rays = torch.empty((max(n, 0), 6), dtype=torch.float64, device=dev)
    lens = abi.lens_params(aperture, focus)
    _check(shim.rt_hip_lens_rays(C.byref(camera), C.byref(lens), width, height, seed, sample, pixel_first, n,
                                 _some(rays), _stream(dev)), "rt_hip_lens_rays")
    return rays


def lens_resolve(total, samples):
    """The lens frame's resolve alone (rt_hip.h, rt_hip_lens_resolve): total float64 [H, W, 3] on a device -> (rgb float32 [H, W, 3],
    rgb8 uint8 [H, W, 3]), the mean over `samples` and its tonemapped bytes; asynchronous on torch's current stream"""
    shim = abi.load_shim()
    total = total.contiguous()
    h, w, _ = total.shape
    rgb, rgb8 = _frame_pair(h, w, total.device)
    _check(shim.rt_hip_lens_resolve(_ptr(total), w, h, samples, _ptr(rgb), _ptr(rgb8), _stream(total.device)), "rt_hip_lens_resolve")
    return rgb, rgb8


def render_lens_host(scene, aperture, focus, samples, seed, camera=None, max_depth=None, device=0):
    """rt_hip_render_lens_image(): the C hosts' entry point (its own scene on logical device `device`, synchronous) ->
    (rgb float32 [H, W, 3], rgb8 uint8 [H, W, 3], stats dict)"""
    shim = abi.load_shim()
    p = _params(scene, seed, samples, _depth(scene, max_depth))
    lens = abi.lens_params(aperture, focus)
    img, img8 = _frame_pair(scene.height, scene.width, None)
    stats = _host_counters()
    _check(shim.rt_hip_render_lens_image(*_host_scene(scene), C.byref(_camera(scene, camera)), C.byref(lens), C.byref(p), device, img.ctypes.data,
                                         img8.ctypes.data, stats), "rt_hip_render_lens_image")
    return img, img8, _stats_dict(stats)


def _origin_radius(r, m, bias):
    """An origin_radius for probes at positions of lengths r (+ normals of lengths m, or None, times bias): the largest finite
    distance from the world's origin, a shade more.  r, m: tensors or numpy arrays [N]."""
    def largest(x):
        x = x[abs(x) < float("inf")]
        return float(x.max()) if len(x) else 0.0
    out = largest(r)
    if m is not None and bias:
        out += bias * largest(m)
    return out * (1.0 + 2.0 ** -40)


def probe_rays(positions, samples, seed, normals=None, bias=0.0, k_first=0, n=None, device=0):
    """The probe rays of indices [k_first, k_first + n) (rt_hip.h, rt_hip_probe_rays; n None: to the end), ray k = probe * samples
    + sample; normals [N, 3]: hemisphere probes, rays flipped to the normal's side and started at position + normal * bias ->
    a device tensor [n, 6] float64 (origin, direction), asynchronous on torch's current stream"""
    shim = abi.load_shim()
    dev = torch.device("cuda", device)
    pos, nrm = _points3(positions, dev), None if normals is None else _points3(normals, dev)
    n = pos.shape[0] * samples - k_first if n is None else n
    rays = torch.empty((max(n, 0), 6), dtype=torch.float64, device=dev)
    p = abi.probe_params(abi.PROBE_SPHERE if nrm is None else abi.PROBE_HEMISPHERE, samples, seed, bias=bias)
    _check(shim.rt_hip_probe_rays(_some(pos), _some(nrm), pos.shape[0], C.byref(p), k_first, n, _some(rays), _stream(dev)), "rt_hip_probe_rays")
    return rays


def probe_resolve(total, samples):
    """A bake's resolve alone (rt_hip.h, rt_hip_probe_resolve): total float64 [N, 9, 3] (sphere probes) or [N, 1, 3] (hemisphere) on
    a device -> (coeff float64, coeff_f float32) of that shape; asynchronous on torch's current stream"""
    shim = abi.load_shim()
    total = total.contiguous()
    n, bases, _ = total.shape
    mode = {9: abi.PROBE_SPHERE, 1: abi.PROBE_HEMISPHERE}[bases]
    coeff, coeff_f = torch.empty_like(total), torch.empty(total.shape, dtype=torch.float32, device=total.device)
    _check(shim.rt_hip_probe_resolve(_ptr(total), n, mode, samples, _ptr(coeff), _ptr(coeff_f), _stream(total.device)), "rt_hip_probe_resolve")
    return coeff, coeff_f


def probe_irradiance(sh, index, normals):
    """Irradiance from SH9 probes (rt_hip.h, rt_hip_probe_irradiance): sh float64 [N, 9, 3] on a device, index [m] (which probe),
    normals [m, 3] (used as given) -> float64 [m, 3]; an index >= N gives NaN; asynchronous on torch's current stream"""
    shim = abi.load_shim()
    sh = sh.contiguous()
    dev = sh.device
    idx = (torch.as_tensor(index, device=dev).to(torch.int64) & 0xFFFFFFFF).to(torch.uint32).reshape(-1).contiguous()
    nrm = _points3(normals, dev)
    m = nrm.shape[0]
    if idx.numel() != m:
        raise ValueError(f"{idx.numel()} indices for {m} normals")
    out = torch.empty((m, 3), dtype=torch.float64, device=dev)
    _check(shim.rt_hip_probe_irradiance(_some(sh), sh.shape[0], _some(idx), _some(nrm), m, _some(out), _stream(dev)), "rt_hip_probe_irradiance")
    return out


def probe_grid_positions(grid, device=0):
    """The positions of a grid's probes in index order (rt_hip.h, rt_hip_probe_grid_positions); grid: abi.probe_grid(...) ->
    float64 [N, 3] on the device, asynchronous on torch's current stream"""
    shim = abi.load_shim()
    dev = torch.device("cuda", device)
    out = torch.empty((_grid_count(grid), 3), dtype=torch.float64, device=dev)
    _check(shim.rt_hip_probe_grid_positions(C.byref(grid), _some(out), _stream(dev)), "rt_hip_probe_grid_positions")
    return out


def probe_shade(grid, coeff, points, normals, status=None, albedo=None, add=None, want=("irradiance", "color"), out=None, m=None, vis=None,
                moments=None):
    """Entries shaded from a grid of SH9 probes (rt_hip.h, rt_hip_probe_shade): coeff float64 [N, 9, 3] on a device, points and
    normals [m, 3] float64 (a ray query's point and normal as they stand), status [m] (the query's words) or None, albedo and add
    [m, 3] float32 or None -> dict of irradiance float64 [m, 3] and color float32 [m, 3] (want: which; out: a dict of tensors to write
    into; m: shade the first m entries only); asynchronous on torch's current stream.  vis (abi.probe_vis(...)) and moments
    [N, R*R, 2]: both or neither; with them every corner is weighed by its visibility (rt_hip_probe_shade_vis)."""
    shim = abi.load_shim()
    if (vis is None) != (moments is None):
        raise ValueError("probe_shade: vis and moments go together")
    coeff = coeff.contiguous()
    dev = coeff.device
    pts, nrm = _points3(points, dev), _points3(normals, dev)
    n = pts.shape[0]
    if nrm.shape[0] != n:
        raise ValueError(f"{nrm.shape[0]} normals for {n} points")
    st = None if status is None else torch.as_tensor(status, device=dev).reshape(-1).contiguous()
    if st is not None and st.dtype not in (torch.int32, torch.uint32):
        st = st.to(torch.int32)
    alb, ad = (None if t is None else _points3(t, dev, torch.float32) for t in (albedo, add))
    for name, t, per in (("status", st, 1), ("albedo", alb, 3), ("add", ad, 3)):
        if t is not None and t.numel() != per * n:
            raise ValueError(f"probe_shade: {name} must hold {per} value(s) per entry")
    res = dict(out) if out is not None else {}
    for f, dt in (("irradiance", torch.float64), ("color", torch.float32)):
        if f in want and f not in res:
            res[f] = torch.empty((n, 3), dtype=dt, device=dev)
    outs = (_some(res.get("irradiance"), "irradiance" in want), _some(res.get("color"), "color" in want), _stream(dev))
    if vis is not None:
        mom = _moments(moments, grid, vis, dev, "probe_shade")
        _check(shim.rt_hip_probe_shade_vis(C.byref(grid), C.byref(vis), _some(coeff), _some(mom), _some(pts), _some(nrm), _some(st), _some(alb),
                                           _some(ad), n if m is None else m, *outs), "rt_hip_probe_shade_vis")
        return {f: res[f] for f in want}
    _check(shim.rt_hip_probe_shade(C.byref(grid), _some(coeff), _some(pts), _some(nrm), _some(st), _some(alb), _some(ad), n if m is None else m,
                                   *outs), "rt_hip_probe_shade")
    return {f: res[f] for f in want}


def _round_count(grid, upd):
    return abi.load_shim().rt_hip_probe_update_count(C.byref(grid), C.byref(upd))


def probe_blend_coeff(total, samples, grid, upd, age, coeff, coeff_f=None, change=None):
    """The coefficient blend of an update round alone (rt_hip.h, rt_hip_probe_blend_coeff): total float64 [M, 9, 3], the fresh sums
    of the round's M probes in their order, blended in place into coeff float64 [N, 9, 3] (coeff_f float32 and change float64 [N]
    where given) by age int32 [N]; device tensors, asynchronous on torch's current stream"""
    dev = age.device
    total = torch.as_tensor(total, dtype=torch.float64, device=dev).contiguous()
    if total.numel() != 27 * _round_count(grid, upd):
        raise ValueError("probe_blend_coeff: total must hold 9 x 3 values per probe of the round")
    _check(abi.load_shim().rt_hip_probe_blend_coeff(_some(total), samples, C.byref(grid), C.byref(upd), _ptr(age), _ptr(coeff), _ptr(coeff_f),
                                                    _ptr(change), _stream(dev)), "rt_hip_probe_blend_coeff")


def probe_blend_moments(sums, grid, vis, upd, age, moments):
    """The moment blend of an update round alone (rt_hip.h, rt_hip_probe_blend_moments): sums float64 [M, R*R, 3] (W, M1, M2 a texel)
    of the round's M probes, blended in place into moments float64 [N, R*R, 2] by age int32 [N]; device tensors, asynchronous"""
    dev = age.device
    sums = torch.as_tensor(sums, dtype=torch.float64, device=dev).contiguous()
    if sums.numel() != 3 * vis.res * vis.res * _round_count(grid, upd):
        raise ValueError("probe_blend_moments: sums must hold R x R x 3 values per probe of the round")
    _check(abi.load_shim().rt_hip_probe_blend_moments(_some(sums), C.byref(grid), C.byref(vis), C.byref(upd), _ptr(age), _ptr(moments),
                                                      _stream(dev)), "rt_hip_probe_blend_moments")


def probe_age_step(grid, upd, age):
    """The age step of an update round alone (rt_hip.h, rt_hip_probe_age_step) on age int32 [N], in place; asynchronous"""
    _check(abi.load_shim().rt_hip_probe_age_step(C.byref(grid), C.byref(upd), _ptr(age), _stream(age.device)), "rt_hip_probe_age_step")


def probe_update_host(scene, grid, upd, samples, seed, coeff, age, vis=None, moments=None, coeff_f=None, change=None, status=None,
                      max_depth=None, origin_radius=None, device=0):
    """rt_hip_probe_grid_update_host(): the C hosts' entry point (its own scene on logical device `device`, synchronous): one update
    round on a state held in numpy arrays, in place -- coeff float64 [N, 9, 3], age uint32 [N], with vis moments float64 [N, R*R, 2];
    coeff_f float32, change float64 [N] and status uint32 [N] where given -> stats dict"""
    shim = abi.load_shim()
    p = abi.probe_params(abi.PROBE_SPHERE, samples, seed, _depth(scene, max_depth), 0.0,
                         _grid_radius(grid) if origin_radius is None else origin_radius)
    stats = _host_counters()
    at = lambda a: None if a is None else a.ctypes.data
    _check(shim.rt_hip_probe_grid_update_host(*_host_scene(scene), C.byref(grid), None if vis is None else C.byref(vis), C.byref(p),
                                              C.byref(upd), device, at(coeff), at(coeff_f), at(moments), at(age), at(change), at(status), stats),
           "rt_hip_probe_grid_update_host")
    return _stats_dict(stats)


def probe_preview_host(scene, grid, samples, seed, camera=None, aov_samples=1, max_depth=None, origin_radius=None, device=0):
    """rt_hip_probe_preview_image(): the C hosts' entry point (its own scene on logical device `device`, synchronous): the grid baked
    with `samples` rays a probe under `seed`, then the preview of the scene's frame -> (rgb float32 [H, W, 3], rgb8 uint8 [H, W, 3],
    coeff float64 [N, 9, 3], stats dict)"""
    shim = abi.load_shim()
    p = abi.probe_params(abi.PROBE_SPHERE, samples, seed, _depth(scene, max_depth), 0.0,
                         _grid_radius(grid) if origin_radius is None else origin_radius)
    img, img8 = _frame_pair(scene.height, scene.width, None)
    coeff = np.zeros((_grid_count(grid), 9, 3), dtype=np.float64)
    stats = _host_counters()
    _check(shim.rt_hip_probe_preview_image(*_host_scene(scene), C.byref(_camera(scene, camera)), C.byref(grid), C.byref(p), scene.width,
                                           scene.height, aov_samples, device, img.ctypes.data, img8.ctypes.data, coeff.ctypes.data, stats),
           "rt_hip_probe_preview_image")
    return img, img8, coeff, _stats_dict(stats)


def probe_preview_vis_host(scene, grid, vis, samples, seed, camera=None, aov_samples=1, max_depth=None, origin_radius=None, device=0):
    """rt_hip_probe_preview_vis_image(): probe_preview_host with the grid's depth moments baked as well and the visibility-weighted
    shade -> (rgb float32 [H, W, 3], rgb8 uint8 [H, W, 3], coeff float64 [N, 9, 3], moments float64 [N, R*R, 2], stats dict)"""
    shim = abi.load_shim()
    p = abi.probe_params(abi.PROBE_SPHERE, samples, seed, _depth(scene, max_depth), 0.0,
                         _grid_radius(grid) if origin_radius is None else origin_radius)
    img, img8 = _frame_pair(scene.height, scene.width, None)
    coeff = np.zeros((_grid_count(grid), 9, 3), dtype=np.float64)
    moments = np.zeros((_grid_count(grid), vis.res * vis.res, 2), dtype=np.float64)
    stats = _host_counters()
    _check(shim.rt_hip_probe_preview_vis_image(*_host_scene(scene), C.byref(_camera(scene, camera)), C.byref(grid), C.byref(vis), C.byref(p),
                                               scene.width, scene.height, aov_samples, device, img.ctypes.data, img8.ctypes.data,
                                               coeff.ctypes.data, moments.ctypes.data, stats), "rt_hip_probe_preview_vis_image")
    return img, img8, coeff, moments, _stats_dict(stats)


def bake_probes_host(scene, positions, samples, seed, normals=None, bias=0.0, max_depth=None, origin_radius=None, device=0):
    """rt_hip_bake_probes_host(): the C hosts' entry point (its own scene on logical device `device`, synchronous); normals None:
    sphere probes -> (coeff float64 [N, 9, 3], coeff_f float32, status uint32 [N], stats dict); with normals: hemisphere probes,
    the arrays [N, 1, 3]"""
    shim = abi.load_shim()
    pos = np.ascontiguousarray(np.asarray(positions, dtype=np.float64).reshape(-1, 3))
    nrm = None if normals is None else np.ascontiguousarray(np.asarray(normals, dtype=np.float64).reshape(-1, 3))
    mode = abi.PROBE_SPHERE if nrm is None else abi.PROBE_HEMISPHERE
    if origin_radius is None:
        norms = lambda a: None if a is None else np.sqrt((a * a).sum(axis=1))
        origin_radius = _origin_radius(norms(pos), norms(nrm), bias)
    p = abi.probe_params(mode, samples, seed, _depth(scene, max_depth), bias, origin_radius)
    n, bases = pos.shape[0], abi.PROBE_BASES[mode]
    coeff = np.zeros((n, bases, 3), dtype=np.float64)
    coeff_f = np.zeros((n, bases, 3), dtype=np.float32)
    status = np.zeros(n, dtype=np.uint32)
    stats = _host_counters()
    _check(shim.rt_hip_bake_probes_host(*_host_scene(scene), pos.ctypes.data, nrm.ctypes.data if nrm is not None else None, n, C.byref(p), device,
                                        coeff.ctypes.data, coeff_f.ctypes.data, status.ctypes.data, stats), "rt_hip_bake_probes_host")
    return coeff, coeff_f, status, _stats_dict(stats)
