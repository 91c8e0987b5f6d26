# Builds the product library (HIP, gfx950 only) and the test oracle (plain C).
#   make            -> oat_amd/lib/liboatgpu.so + oracle/liboat_oracle.so
#   make host       -> C++ drop-in binaries under build/bin
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
# -ffp-contract=off is a PARITY requirement (the reference's CPU build rounds every
# mul/add of the MOG2 update separately), not a tuning choice.
HIPFLAGS ?= --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -fPIC -Wall -Wno-unused-result -Wno-unused-value
CSRC     = oat_amd/csrc
LIB      = oat_amd/lib/liboatgpu.so
# the units of the library, listed once: the kernels, and the C ABI above them by feature (oatgpu_ctx.h is their shared header)
KERNELS  = kernels_mog kernels_stages kernels_measure kernels_rowscan kernels_bloblds kernels_blob kernels_kalman kernels_undistort kernels_debayer kernels_markers kernels_diff kernels_bsubtrack kernels_trackfilt kernels_tracks kernels_crops kernels_croptensor kernels_targetmask
API      = api_context api_stages api_track api_markers api_diff api_bsubtrack api_trackfilt api_targets api_tracks api_crops api_croptensor api_targetmask api_model api_measure
UNITS    = $(KERNELS) $(API)
OBJS     = $(UNITS:%=$(CSRC)/%.o)

all: $(LIB) oracle

# every unit depends on every header of the directory: a new header is a dependency without being listed
$(CSRC)/%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.h) include/oatgpu.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p oat_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)
	python3 tools/isa_hazard_check.py $@      # the gfx950 wide-store data hazard: the binary is checked, DESIGN.md 3b

oracle:
	$(MAKE) -C oracle

host: $(LIB) tools
	$(MAKE) -C oat_amd/host

# measurement aids: the pipelined loop from a plain C++ process, and a launch/event cost microbenchmark
tools: build/bin/bench_native build/bin/launch_gap
build/bin/bench_native: tools/bench_native.hip include/oatgpu.h $(LIB)
	@mkdir -p build/bin
	$(HIPCC) --offload-arch=$(ARCH) -O2 -w $< -Iinclude -Loat_amd/lib -loatgpu -Wl,-rpath,'$$ORIGIN/../../oat_amd/lib' -o $@
build/bin/launch_gap: tools/launch_gap.hip
	@mkdir -p build/bin
	$(HIPCC) --offload-arch=$(ARCH) -O2 -w $< -o $@

clean:
	rm -f $(OBJS) $(LIB)
	$(MAKE) -C oracle clean

.PHONY: all oracle host tools clean

# A/B variant builds: make variant NAME=px2 DEFS="-DOATGPU_PX=2"  -> build/variants/liboatgpu_px2.so
# Only these builds (-DOATGPU_MEASURE) read the OATGPU_A_RESERVE / EARLY_BLOB / EARLY_MIN_PX / LONE_PLAIN / PAIR_BACK /
# K1_WG / K1_STOP_EVENT / K1_LDS / RS_DEEP_ROWS measurement switches from the environment; the product library ignores them.
# They live under build/ (git-ignored, but they travel to the GPU box):
# oat_amd/lib/ holds the product library and nothing else, and the Python binding loads another library only with
# OATGPU_MEASURE_PY=1 OATGPU_LIB=<path> (oat_amd/ffi.py; the tools/*.sh A/B scripts set both).
variant:
	@mkdir -p build/$(NAME) build/variants
	for f in $(UNITS); do $(HIPCC) $(HIPFLAGS) -DOATGPU_MEASURE $(DEFS) -c $(CSRC)/$$f.hip -o build/$(NAME)/$$f.o || exit 1; done
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o build/variants/liboatgpu_$(NAME).so build/$(NAME)/*.o
clean-variants:
	rm -rf build/variants oat_amd/lib/liboatgpu_*.so
.PHONY: variant clean-variants
