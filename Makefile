# Builds libdmip.so (gfx950) in-tree. Used by __graft_entry__.build(); `make -j2` by hand.
PKG := diffusion-modelling-for-inverse-problems_amd
CSRC := $(PKG)/csrc
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-parameter
F32OBJS := $(CSRC)/dmip_f32.o $(CSRC)/dmip_f32_cde.o $(CSRC)/dmip_f32_post.o $(CSRC)/dmip_f32_cdiffe.o $(CSRC)/dmip_flow.o \
           $(CSRC)/dmip_f32_cde_heun.o $(CSRC)/dmip_f32_post_heun.o $(CSRC)/dmip_flow_sample.o \
           $(CSRC)/dmip_dps_linear.o $(CSRC)/dmip_f32_cde_ms.o $(CSRC)/dmip_f32_post_ms.o \
           $(CSRC)/dmip_f32_cde_ms_sde.o $(CSRC)/dmip_f32_post_ms_sde.o \
           $(CSRC)/dmip_flow_pairs.o $(CSRC)/dmip_flow_sample_pairs.o $(CSRC)/dmip_dps_tweedie.o
X3OBJS := $(CSRC)/dmip_x3.o $(CSRC)/dmip_x3_cde.o $(CSRC)/dmip_x3_post.o $(CSRC)/dmip_x3_cdiffe.o $(CSRC)/dmip_x3k.o \
          $(CSRC)/dmip_dps_x3.o $(CSRC)/dmip_x3_cde_heun.o $(CSRC)/dmip_x3_post_heun.o \
          $(CSRC)/dmip_x3_flow.o $(CSRC)/dmip_x3_flow_cde.o $(CSRC)/dmip_x3_flow_post.o \
          $(CSRC)/dmip_x3_flow_sample_cde.o $(CSRC)/dmip_x3_flow_sample_post.o $(CSRC)/dmip_x3_dps_linear.o \
          $(CSRC)/dmip_x3_cde_ms.o $(CSRC)/dmip_x3_post_ms.o $(CSRC)/dmip_x3_cde_ms_sde.o $(CSRC)/dmip_x3_post_ms_sde.o \
          $(CSRC)/dmip_x3_flow_pairs.o $(CSRC)/dmip_x3_flow_pairs_cde.o $(CSRC)/dmip_x3_flow_pairs_post.o \
          $(CSRC)/dmip_x3_flow_sample_pairs_cde.o $(CSRC)/dmip_x3_flow_sample_pairs_post.o $(CSRC)/dmip_x3_dps_tweedie.o
# the host sources: the C-ABI layer by concern (handles and upload, sampling entry points, the probability-flow entry
# points, training entry points, linear guided sampling) and the weight packers (pure host code, dmip_pack.h)
CAPI := dmip_capi_pack dmip_capi_sample dmip_capi_flow dmip_capi_train dmip_capi_dps_linear dmip_pack
CAPIOBJS := $(patsubst %,$(CSRC)/%.o,$(CAPI))
OBJS := $(CSRC)/dmip_kernels.o $(CSRC)/dmip_train.o $(CSRC)/dmip_eval.o $(CSRC)/dmip_surrogate.o $(CSRC)/dmip_gemm.o $(CSRC)/dmip_jets.o $(CSRC)/dmip_step.o $(F32OBJS) $(X3OBJS) $(CAPIOBJS)
HDRS := $(CSRC)/dmip_device.h $(CSRC)/dmip_internal.h include/dmip.h

all: $(PKG)/libdmip.so

# no SLP vectorisation in the sampler: packed f32 FMAs (v_pk_fma_f32) beside MFMAs cost more than
# the scalar pair (MI355X_MICROARCH.md, filler prices); bf16 packing is written out pairwise instead
$(CSRC)/dmip_kernels.o: $(CSRC)/dmip_kernels.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

$(CSRC)/dmip_train.o: $(CSRC)/dmip_train.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/dmip_eval.o: $(CSRC)/dmip_eval.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/dmip_surrogate.o: $(CSRC)/dmip_surrogate.hip $(CSRC)/dmip_mh_chains.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/dmip_gemm.o: $(CSRC)/dmip_gemm.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/dmip_jets.o: $(CSRC)/dmip_jets.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/dmip_step.o: $(CSRC)/dmip_step.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# exact-f32 parity engine: one header, four translation units compiled in parallel
$(CSRC)/dmip_f32.o: $(CSRC)/dmip_f32.hip $(CSRC)/dmip_f32.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/dmip_f32_%.o: $(CSRC)/dmip_f32_%.hip $(CSRC)/dmip_f32.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# log p(x | y) along the probability-flow ODE, on the exact-f32 engine's header
$(CSRC)/dmip_flow.o: $(CSRC)/dmip_flow.hip $(CSRC)/dmip_flow.h $(CSRC)/dmip_flow_rows.h $(CSRC)/dmip_f32.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# samples with their log-density: the Heun sampler's steps with the log-likelihood kernel's tangent columns
$(CSRC)/dmip_flow_sample.o: $(CSRC)/dmip_flow_sample.hip $(CSRC)/dmip_flow.h $(CSRC)/dmip_flow_rows.h $(CSRC)/dmip_f32.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# guided sampling for linear problems from a prior alone (dmip_flow_rows.h dps_linear_rows), exact f32
$(CSRC)/dmip_dps_linear.o: $(CSRC)/dmip_dps_linear.hip $(CSRC)/dmip_flow.h $(CSRC)/dmip_flow_rows.h $(CSRC)/dmip_f32.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the same sampler with the Tweedie-covariance guidance (dps_linear_rows over DpsTweedieChains), exact f32
$(CSRC)/dmip_dps_tweedie.o: $(CSRC)/dmip_dps_tweedie.hip $(CSRC)/dmip_flow.h $(CSRC)/dmip_flow_rows.h $(CSRC)/dmip_f32.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the paired flow kernels (one observation per row), exact f32: dmip_flow.h's network with a per-row layer-1 bias
PAIRSHDRS := $(CSRC)/dmip_pairs.h $(CSRC)/dmip_flow_rows.h $(HDRS)
$(CSRC)/dmip_flow_pairs.o $(CSRC)/dmip_flow_sample_pairs.o: $(CSRC)/%.o: $(CSRC)/%.hip $(CSRC)/dmip_flow_pairs.h $(CSRC)/dmip_flow.h $(CSRC)/dmip_f32.h $(PAIRSHDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# fp32-accurate split-fp16 engine (DMIP_PREC_F32X3): one header, four translation units; no SLP
# vectorisation (it packs the split's f32 subtractions into v_pk_add_f32, an anti-lever beside MFMAs)
$(CSRC)/dmip_x3.o: $(CSRC)/dmip_x3.hip $(CSRC)/dmip_x3.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

$(CSRC)/dmip_x3_%.o: $(CSRC)/dmip_x3_%.hip $(CSRC)/dmip_x3.h $(CSRC)/dmip_x3s.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

# log p(x | y) and samples with their log-density on the fp32x3 engine: free functions beside it (dmip_x3_flow.h),
# the dispatch and four translation units of instantiations
$(CSRC)/dmip_x3_flow.o: $(CSRC)/dmip_x3_flow.hip $(CSRC)/dmip_x3_flow.h $(CSRC)/dmip_flow_rows.h $(CSRC)/dmip_x3.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

$(CSRC)/dmip_x3_flow_%.o: $(CSRC)/dmip_x3_flow_%.hip $(CSRC)/dmip_x3_flow.h $(CSRC)/dmip_flow_rows.h $(CSRC)/dmip_x3.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

# the paired flow kernels on the fp32x3 engine: the dispatch and four translation units of instantiations (static
# pattern rules: they beat dmip_x3_flow_%.o)
$(CSRC)/dmip_x3_flow_pairs.o: $(CSRC)/dmip_x3_flow_pairs.hip $(PAIRSHDRS)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

X3PAIRS := dmip_x3_flow_pairs_cde dmip_x3_flow_pairs_post dmip_x3_flow_sample_pairs_cde dmip_x3_flow_sample_pairs_post
$(patsubst %,$(CSRC)/%.o,$(X3PAIRS)): $(CSRC)/%.o: $(CSRC)/%.hip $(CSRC)/dmip_x3_flow_pairs.h $(CSRC)/dmip_x3_flow.h $(CSRC)/dmip_x3.h $(PAIRSHDRS)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

# the same on the fp32x3 engine (listed before nothing else matches it: an explicit rule beats dmip_x3_%.o)
$(CSRC)/dmip_x3_dps_linear.o: $(CSRC)/dmip_x3_dps_linear.hip $(CSRC)/dmip_x3_flow.h $(CSRC)/dmip_flow_rows.h $(CSRC)/dmip_x3.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

# the Tweedie-covariance guidance on the fp32x3 engine (explicit, as dmip_x3_dps_linear.o)
$(CSRC)/dmip_x3_dps_tweedie.o: $(CSRC)/dmip_x3_dps_tweedie.hip $(CSRC)/dmip_x3_flow.h $(CSRC)/dmip_flow_rows.h $(CSRC)/dmip_x3.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

# the k-major multi-tile fp32x3 CDE engine (width 256): its own header
$(CSRC)/dmip_x3k.o: $(CSRC)/dmip_x3k.hip $(CSRC)/dmip_x3k.h $(CSRC)/dmip_x3.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

# DPS (config 4) on the split-fp16 arithmetic
$(CSRC)/dmip_dps_x3.o: $(CSRC)/dmip_dps_x3.hip $(CSRC)/dmip_mh_chains.h $(CSRC)/dmip_x3.h $(HDRS)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

CAPIHDRS := $(CSRC)/dmip_capi_common.h $(CSRC)/dmip_pack.h $(CSRC)/dmip_pairs.h $(HDRS)
$(CAPIOBJS): $(CSRC)/%.o: $(CSRC)/%.cpp $(CAPIHDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(PKG)/libdmip.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(OBJS) -o $@

# A/B + diagnostic library (never the product): the samplers' timing ablations and per-phase cycle stamps behind
# -DDMIP_DIAG (run-time DMIP_X3_DIAG for the x3 / x3k engines, scripts/x3k_stamps.py), and the paired-tile 32x32
# fp32x3 engine (dmip_x3p.h, opt-in DMIP_X3P=1; it measured slower than x3k, so libdmip.so does not hold it).
# Load it with DMIP_LIB=abv/diag/libdmip_diag.so (tests/test_gpu_x3p.py runs there). The paired engine's
# per-chunk stamps (scripts/x3p_stamps.py) replace its snapshots, so they need their own build:
# make diag X3P_DIAG=-DDMIP_X3P_DIAG
DIAG_DIR := abv/diag
DIAG_SRCS := dmip_x3_cde dmip_x3k dmip_capi_pack dmip_capi_sample dmip_pack
diag: $(DIAG_DIR)/libdmip_diag.so
$(DIAG_DIR)/%_diag.o: $(CSRC)/%.hip $(CSRC)/dmip_x3k.h $(CSRC)/dmip_x3.h $(CSRC)/dmip_x3s.h $(HDRS)
	@mkdir -p $(DIAG_DIR)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -DDMIP_DIAG -c $< -o $@
X3P_DIAG ?=
$(DIAG_DIR)/dmip_x3p_diag.o: $(CSRC)/dmip_x3p.hip $(CSRC)/dmip_x3p.h $(CSRC)/dmip_x3.h $(HDRS)
	@mkdir -p $(DIAG_DIR)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize $(X3P_DIAG) -c $< -o $@
# the paired engine's packer (dmip_pack.cpp), its upload (dmip_capi_pack.cpp) and its launch (dmip_capi_sample.cpp)
$(DIAG_DIR)/%_diag.o: $(CSRC)/%.cpp $(CAPIHDRS)
	@mkdir -p $(DIAG_DIR)
	$(HIPCC) $(HIPFLAGS) -DDMIP_WITH_X3P -c $< -o $@
$(DIAG_DIR)/libdmip_diag.so: $(filter-out $(patsubst %,$(CSRC)/%.o,$(DIAG_SRCS)),$(OBJS)) $(patsubst %,$(DIAG_DIR)/%_diag.o,$(DIAG_SRCS)) $(DIAG_DIR)/dmip_x3p_diag.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@

# microbenchmarks (scripts/ubench): built here, never committed
UBENCH := scripts/ubench/valu_mix scripts/ubench/valu_rates
ubench: $(UBENCH)
scripts/ubench/%: scripts/ubench/%.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 $< -o $@

# Host-only AddressSanitizer build of the C-ABI layer (argument validation, packing, handle
# management): every dmip_capi_*.cpp instrumented as host code, linked with the same kernel objects,
# driven by tests/asan/capi_args.cpp through the calls that need no GPU.
# The capi sources have no device code: they compile as plain host C++ against the HIP runtime headers.
ASAN_DIR := build/asan
HOSTCXX ?= /opt/rocm/lib/llvm/bin/clang++
ASANFLAGS := -O1 -g -std=c++17 -fPIC -fsanitize=address -fno-omit-frame-pointer
HOSTINC := -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
# the packers' program (tests/pack/pack_images.cpp, below) joins where a tree carries it; capi_args needs no more than
# tests/asan/capi_args.cpp, as before
asan: $(ASAN_DIR)/capi_args $(if $(wildcard tests/pack/pack_images.cpp),$(ASAN_DIR)/pack_images)
$(ASAN_DIR)/%_asan.o: $(CSRC)/%.cpp $(CAPIHDRS)
	@mkdir -p $(ASAN_DIR)
	$(HOSTCXX) -x c++ $(HOSTINC) $(ASANFLAGS) -c $< -o $@
$(ASAN_DIR)/libdmip_asan.so: $(filter-out $(CAPIOBJS),$(OBJS)) $(patsubst %,$(ASAN_DIR)/%_asan.o,$(CAPI))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -fsanitize=address $^ -o $@
$(ASAN_DIR)/capi_args: tests/asan/capi_args.cpp $(ASAN_DIR)/libdmip_asan.so include/dmip.h
	$(HOSTCXX) $(ASANFLAGS) $< -L$(ASAN_DIR) -ldmip_asan -Wl,-rpath,$(abspath $(ASAN_DIR)) -lpthread -o $@

# The packers without a GPU (tests/test_pack_images.py, tests/golden/pack_images.md): tests/pack/pack_images.cpp prints
# a hash of every image dmip_pack.cpp makes of a few small networks. Compiled with the paired engine's packer; linked
# with the library for the kernels' layout constants. `make asan` builds the same program under AddressSanitizer.
PACK_DIR := build/pack
PACKSRCS := tests/pack/pack_images.cpp $(CSRC)/dmip_pack.cpp
PACKFLAGS := $(HOSTINC) -std=c++17 -ffp-contract=off -DDMIP_WITH_X3P
packcheck: $(PACK_DIR)/pack_images
	@$<
$(PACK_DIR)/pack_images: $(PACKSRCS) $(CAPIHDRS) $(PKG)/libdmip.so
	@mkdir -p $(PACK_DIR)
	$(HOSTCXX) $(PACKFLAGS) -O3 $(PACKSRCS) -L$(PKG) -ldmip -Wl,-rpath,$(abspath $(PKG)) -lpthread -o $@
$(ASAN_DIR)/pack_images: $(PACKSRCS) $(CAPIHDRS) $(ASAN_DIR)/libdmip_asan.so
	$(HOSTCXX) $(PACKFLAGS) $(ASANFLAGS) $(PACKSRCS) -L$(ASAN_DIR) -ldmip_asan -Wl,-rpath,$(abspath $(ASAN_DIR)) -lpthread -o $@

clean:
	rm -f $(OBJS) $(PKG)/libdmip.so $(UBENCH)
	rm -rf $(ASAN_DIR) $(PACK_DIR)

.PHONY: all clean ubench asan diag packcheck
