# Top-level build.  Everything is built IN-TREE so the binaries travel to the GPU box
# with the source snapshot (they are git-ignored, not gpurun-ignored).
#
#   make            shim + its PT_DIAG twin + its development build + its PT_DIR_PARK=0 and PT_MFMA16=0 twins (the latter also as PT_DIAG) + host library + CLI + oracle checkers
#   make shim       raytracer.c_amd/csrc/librt_hip.so        (hipcc, gfx950 only)
#   make host       raytracer.c_amd/host/libraytracer_amd.so + raytracer (gcc, C99)
#   make oracle     oracle/libpt_oracle.so (+ oracle/_ref/*.so when /root/reference exists)

ROOT    := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
PKG     := $(ROOT)raytracer.c_amd
CSRC    := $(PKG)/csrc
HOST    := $(PKG)/host
INC     := $(ROOT)include

HIPCC   ?= /opt/rocm/bin/hipcc
# -ffp-contract=off: decision-exact parity with the reference (gcc --std=c99 emits no FMA);
# hipcc's default would fuse a*b+c.  No fast-math: IEEE fp64 sqrt and division.
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Wall -Wno-unused-function \
            -I$(INC) -I$(CSRC)
CC      := gcc
CFLAGS  := -std=c99 -D_DEFAULT_SOURCE -O2 -ffp-contract=off -fPIC -Wall -Wno-unused-function -I$(INC) -I$(HOST)

SHIM    := $(CSRC)/librt_hip.so
# the path tracer's device code is one translation unit, pt_kernel.hip, split by topic into the pt_*.h headers it includes; the
# hierarchy build, the scene updates, the lens, the image-space passes and the light probes are a translation unit each
# the seven sources every build of the shim compiles, in this order
SHIM_SRC := $(CSRC)/pt_kernel.hip $(CSRC)/rt_hip_shim.hip $(CSRC)/bvh_device.hip $(CSRC)/scene_update.hip $(CSRC)/lens.hip \
            $(CSRC)/image_ops.hip $(CSRC)/probe.hip
KERNEL_SRC := $(SHIM_SRC) $(wildcard $(CSRC)/pt_*.h) $(CSRC)/bvh_build.h $(CSRC)/scene_spheres.h $(CSRC)/scene_materials.h $(CSRC)/ray_store.h $(CSRC)/rt_staging.h $(INC)/rt_hip.h $(INC)/rt_rng.h
HOSTLIB := $(HOST)/libraytracer_amd.so
CLI     := $(HOST)/raytracer

HOST_SRC := $(HOST)/raytracer_amd.c $(HOST)/scenes.c $(HOST)/obj_load.c $(HOST)/png_out.c
HOST_HDR := $(INC)/raytracer.h $(INC)/vector.h $(INC)/rt_hip.h $(INC)/rt_rng.h $(HOST)/scenes.h

all: shim shim-diag shim-dev shim-park0 shim-mfma0 shim-diag-mfma0 host oracle

# oracle/_ref/ref_main_dropin links against the host library: build that first
oracle: host

shim: $(SHIM)
$(SHIM): $(KERNEL_SRC)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(SHIM_SRC) -lrccl

# diagnostic build: wave-level event counters in stats[4..] and the exhaustive re-checks of every conservative rule
# (filter, fp32 pre-tests, bounding-sphere probe, hull facets).  Not the product: only tests/test_gpu_diag.py
# (child processes with RT_HIP_SHIM_PATH) and tools/diag*.py load it.  Built by `make all` so that it travels to
# the GPU box with the snapshot like the other binaries (git-ignored, not gpurun-ignored).
shim-diag: $(CSRC)/librt_hip_diag.so
$(CSRC)/librt_hip_diag.so: $(KERNEL_SRC)
	$(HIPCC) $(HIPFLAGS) -DPT_DIAG -shared -o $@ $(SHIM_SRC) -lrccl

# development build (-DPT_DEV_KERNELS): the product plus what only A/B runs and tests of the fallbacks need -- pt_render_tiles_v0
# (the literal single-phase scan), RT_HIP_KERNEL_VARIANT (other arms of the pick table), RT_HIP_FORCE_BIG, RT_HIP_NO_BIG_PRUNE,
# RT_HIP_EXTRA_LDS, RT_HIP_BVH_MEDIAN, RT_HIP_POOL_SLOTS (pools of n slots per XCD: n = 1 makes slot acquisition FAIL, which is
# how the status-word path is tested).  None of these switches exists in librt_hip.so.  Loaded through RT_HIP_SHIM_PATH by
# child processes of the tests and by tools/; built by `make all` so that it travels to the GPU box with the snapshot.
shim-dev: $(CSRC)/librt_hip_dev.so
$(CSRC)/librt_hip_dev.so: $(KERNEL_SRC)
	$(HIPCC) $(HIPFLAGS) -DPT_DEV_KERNELS -shared -o $@ $(SHIM_SRC) -lrccl

# the A/B knob's other arm (-DPT_DIR_PARK=0: direction retries carried in their lane, four rounds a trip, as before the retry
# stack).  Not the product: tests/test_gpu_dir_park.py renders one case with it in a child process and asks for the shipped
# build's frame bit for bit, and tools/gpu_ab.py times it.  Built by `make all` so that it travels with the snapshot.
shim-park0: $(CSRC)/variants/librt_hip_park0.so
$(CSRC)/variants/librt_hip_park0.so: $(KERNEL_SRC)
	@mkdir -p $(CSRC)/variants
	$(HIPCC) $(HIPFLAGS) -DPT_DIR_PARK=0 -shared -o $@ $(SHIM_SRC) -lrccl

# the other arm of the matrix-pipe filter's A/B (-DPT_MFMA16=0: phase 1 of every sphere in the packed-fp32 loop).  Not the product:
# tests/test_gpu_mfma16.py renders with it in a child process and asks for the shipped build's frames and counters bit for bit, and
# tools/gpu_ab.py times it.  Built by `make all` so that it travels with the snapshot.
shim-mfma0: $(CSRC)/variants/librt_hip_mfma0.so
$(CSRC)/variants/librt_hip_mfma0.so: $(KERNEL_SRC)
	@mkdir -p $(CSRC)/variants
	$(HIPCC) $(HIPFLAGS) -DPT_MFMA16=0 -shared -o $@ $(SHIM_SRC) -lrccl

# the diagnostic build of that arm: tests/test_gpu_mfma16.py compares the two diagnostic builds' candidate counts (what the matrix
# pipe keeps and the packed loop drops, per filter evaluation)
shim-diag-mfma0: $(CSRC)/variants/librt_hip_diag_mfma0.so
$(CSRC)/variants/librt_hip_diag_mfma0.so: $(KERNEL_SRC)
	@mkdir -p $(CSRC)/variants
	$(HIPCC) $(HIPFLAGS) -DPT_DIAG -DPT_MFMA16=0 -shared -o $@ $(SHIM_SRC) -lrccl

host: $(HOSTLIB) $(CLI)
$(HOSTLIB): $(HOST_SRC) $(HOST_HDR) $(SHIM)
	$(CC) $(CFLAGS) -shared -o $@ $(HOST_SRC) -L$(CSRC) -lrt_hip -Wl,-rpath,'$$ORIGIN/../csrc' -lz -lm
$(CLI): $(HOST)/main.c $(HOSTLIB)
	$(CC) $(CFLAGS) -o $@ $(HOST)/main.c -L$(HOST) -lraytracer_amd -L$(CSRC) -lrt_hip -Wl,-rpath,'$$ORIGIN' \
	    -Wl,-rpath,'$$ORIGIN/../csrc' -lm

oracle:
	$(MAKE) -C $(ROOT)oracle all

clean:
	rm -f $(SHIM) $(CSRC)/librt_hip_diag.so $(CSRC)/librt_hip_dev.so $(CSRC)/variants/librt_hip_park0.so $(CSRC)/variants/librt_hip_mfma0.so $(CSRC)/variants/librt_hip_diag_mfma0.so $(CSRC)/variants/librt_hip_gather.so $(HOSTLIB) $(CLI)
	$(MAKE) -C $(ROOT)oracle clean

.PHONY: all shim shim-diag shim-dev shim-park0 shim-mfma0 shim-diag-mfma0 host oracle clean

# development: alternative builds of the shim for A/B runs (tools/gpu_ab.py), e.g.
#   make variant NAME=tri4 DEFS="-DPT_MIN_WAVES_TRI=4"   ->  raytracer.c_amd/csrc/variants/librt_hip_tri4.so
variant:
	@mkdir -p $(CSRC)/variants
	$(HIPCC) $(HIPFLAGS) $(DEFS) -shared -o $(CSRC)/variants/librt_hip_$(NAME).so $(SHIM_SRC) -lrccl
.PHONY: variant
