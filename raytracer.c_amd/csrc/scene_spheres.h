/* scene_spheres.h -- what a scene derives from its spheres: scene_sphere_entry, the parts of the scalars that are maxima,
 * scene_sphere_leading_walls, and scene_sphere_bounds, the sequential statement of all of it.  The text itself stands in
 * bvh_build.h, next to scene_triangle_entry, its twin for the triangles: rt_hip_shim.hip includes that file, and the benchmark's
 * source hash (bench.py, KERNEL_SOURCES) covers exactly the files the shim and the kernels include -- a record under profiles/
 * is tied to this text too.  This header is the name under which scene_update.hip and the CPU harness of the sphere update
 * (tests/sphere_update_harness.cpp) take it. */
#ifndef SCENE_SPHERES_H
#define SCENE_SPHERES_H

#include "bvh_build.h"

#endif /* SCENE_SPHERES_H */
