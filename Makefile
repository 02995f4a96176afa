# Builds the gfx950 shared library (the C ABI of include/myraytracer_amd.h), the headless
# CLI, and the CPU oracle.  `python -c "import __graft_entry__ as g; g.build()"` runs this.
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
CSRC     := myraytracer_amd/csrc
LIBDIR   := myraytracer_amd/lib
LIB      := $(LIBDIR)/libmyraytracer_amd.so
CLI      := $(LIBDIR)/native_runner
# the failure-injecting build of the same sources (test infrastructure: tests/failinject/, tests/test_gpu_failure_paths.py)
FI_DIR   := tests/failinject
FI_LIB   := $(LIBDIR)/libmyraytracer_amd_failinject.so
# -ffp-contract=off: fma only where the source says fma (MRT-F32 rules).
# -fno-vectorize -fno-slp-vectorize: v_pk_* fp32 is not faster than scalar VALU on gfx950
# and SLP packing spends s_mov on SGPR pairs (profiles/r01_ubench_sphere_loop_*.txt).
# -mllvm -amdgpu-mfma-vgpr-form: the matrix-core sweep reads its MFMA results with VALU ops; in AGPRs
# every value would cost a v_accvgpr_read first.
HIPFLAGS := -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -ffp-contract=off -fno-vectorize -fno-slp-vectorize -mllvm -amdgpu-mfma-vgpr-form -Wall -Wextra -Wno-unused-parameter
# the sources and headers: scripts/source_hash.py holds the one list (the build id is the hash over the same files)
SRCS     := $(shell python3 scripts/source_hash.py --srcs)
HDRS     := $(shell python3 scripts/source_hash.py --hdrs)
ifeq ($(strip $(SRCS)),)
$(error scripts/source_hash.py --srcs printed no sources)
endif

all: $(LIB) $(CLI) $(FI_LIB) oracle

# one object per source (build/ is git-ignored), so that touching the host code does not recompile the kernels
OBJDIR   := build/obj
OBJS     := $(patsubst $(CSRC)/%,$(OBJDIR)/%.o,$(SRCS))

$(OBJDIR)/%.o: $(CSRC)/% $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -x hip -c -o $@ $<

# the ISA check (scalar-load hazards of the hand-issued s_loads) gates the link
$(OBJDIR)/isa.ok: $(CSRC)/kernels.hip $(HDRS) scripts/check_isa.py
	@mkdir -p $(OBJDIR)
	python3 scripts/check_isa.py
	@touch $@

# mrt_build_id(): the sha256 over the sources (scripts/source_hash.py), regenerated whenever one of them changes
$(OBJDIR)/build_id.cpp: $(SRCS) $(HDRS) Makefile scripts/source_hash.py
	@mkdir -p $(OBJDIR)
	python3 scripts/source_hash.py --cpp > $@

$(LIB): $(OBJS) $(OBJDIR)/isa.ok $(OBJDIR)/build_id.cpp
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -fPIC -shared -o $@ $(OBJS) $(OBJDIR)/build_id.cpp -ldl

# The failure-injecting library: the host .cpp files compiled once more with tests/failinject/mrt_failinject.h force-included
# (their resource creators / releasers, copies and memsets go through the shim), the product's kernel objects as they are, and
# the shim.  Selected at run time by MRT_LIB_OVERRIDE (bench.py refuses a headline from it); never the product.
FI_OBJDIR := $(OBJDIR)/failinject
FI_HOST   := $(filter %.cpp,$(SRCS))
FI_OBJS   := $(patsubst $(CSRC)/%,$(FI_OBJDIR)/%.o,$(FI_HOST))
KERNEL_OBJS := $(patsubst $(CSRC)/%,$(OBJDIR)/%.o,$(filter-out %.cpp,$(SRCS)))

$(FI_OBJDIR)/%.o: $(CSRC)/% $(HDRS) $(FI_DIR)/mrt_failinject.h
	@mkdir -p $(FI_OBJDIR)
	$(HIPCC) $(HIPFLAGS) -include $(FI_DIR)/mrt_failinject.h -x hip -c -o $@ $<

$(FI_OBJDIR)/shim.o: $(FI_DIR)/mrt_failinject.cpp $(FI_DIR)/mrt_failinject.h
	@mkdir -p $(FI_OBJDIR)
	$(HIPCC) -O2 -std=c++17 -fPIC -Wall -Wextra -x hip --offload-arch=$(ARCH) -c -o $@ $<

$(FI_LIB): $(FI_OBJS) $(FI_OBJDIR)/shim.o $(KERNEL_OBJS) $(OBJDIR)/isa.ok $(OBJDIR)/build_id.cpp
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -fPIC -shared -o $@ $(FI_OBJS) $(FI_OBJDIR)/shim.o $(KERNEL_OBJS) $(OBJDIR)/build_id.cpp -ldl

$(CLI): $(CSRC)/native_runner.cpp $(LIB)
	$(HIPCC) -O2 -std=c++17 -o $@ $(CSRC)/native_runner.cpp -L$(LIBDIR) -lmyraytracer_amd -Wl,-rpath,'$$ORIGIN'

oracle:
	$(MAKE) -s -C oracle

clean:
	rm -rf $(LIBDIR) $(OBJDIR)
	$(MAKE) -s -C oracle clean

.PHONY: all oracle clean

# diagnostic build with s_memtime phase stamps (scripts/phase_profile.py); not the product
stamps: $(SRCS) $(HDRS) $(OBJDIR)/build_id.cpp
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -DMRT_STAMPS -shared -o $(LIBDIR)/libmyraytracer_amd_stamps.so $(SRCS) $(OBJDIR)/build_id.cpp -ldl

# the same with the tail split into primary hit / shading / rejection loop / scatter + normalize instead of the walk's phases
# (-DMRT_STAMPS=2, kernels.hip; scripts/cam_list_profile.py ... tail, scripts/phase_profile.py with MRT_STAMPS_TAIL=1)
stamps-tail: $(SRCS) $(HDRS) $(OBJDIR)/build_id.cpp
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -DMRT_STAMPS=2 -shared -o $(LIBDIR)/libmyraytracer_amd_stamps_tail.so $(SRCS) $(OBJDIR)/build_id.cpp -ldl

# experiment builds (never the product): make variant NAME=slots16 FLAGS="-DMRT_MAX_SLOTS=16" -> lib/libmyraytracer_amd_slots16.so,
# selected at run time by MRT_LIB_OVERRIDE (bench.py refuses a headline from it)
variant: $(SRCS) $(HDRS) $(OBJDIR)/build_id.cpp
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) $(FLAGS) -shared -o $(LIBDIR)/libmyraytracer_amd_$(NAME).so $(SRCS) $(OBJDIR)/build_id.cpp -ldl
