/* scene_materials.h -- what a scene derives from its materials: scene_material_ok (the acceptance rule), scene_material_record
 * (the record of PT_MAT_STRIDE doubles), the parts of the four scalars (scene_material_emission_part, scene_material_class_part)
 * and scene_material_bounds, the sequential statement of all of it.  The text itself stands in bvh_build.h, next to the spheres'
 * and the triangles': rt_hip_shim.hip includes that file, and the benchmark's source hash (bench.py, KERNEL_SOURCES) covers
 * exactly the files the shim and the kernels include -- a record under profiles/ is tied to this text too.  This header is the
 * name under which scene_update.hip and the CPU harness of the material update (tests/material_harness.cpp) take it. */
#ifndef SCENE_MATERIALS_H
#define SCENE_MATERIALS_H

#include "bvh_build.h"

#endif /* SCENE_MATERIALS_H */
