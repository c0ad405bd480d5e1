# Builds libsvc_hip.so (gfx950) in-tree. Usage: make -j8
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
SRC_DIR := svc_inference_pipeline_amd/csrc
SRCS := $(wildcard $(SRC_DIR)/*.hip)
OBJS := $(patsubst $(SRC_DIR)/%.hip,build/%.o,$(SRCS))
LIB := svc_inference_pipeline_amd/libsvc_hip.so
CXXFLAGS := -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall -Wno-unused-function -Wno-unused-variable \
            -Iinclude -I$(SRC_DIR)

all: $(LIB)

build/%.o: $(SRC_DIR)/%.hip $(wildcard $(SRC_DIR)/*.h) include/svc_hip.h
	@mkdir -p build
	$(HIPCC) $(CXXFLAGS) -c $< -o $@

# attention's softmax maxima: no NaN reaches them (masked keys are -inf), so the compiler need not canonicalise every
# MFMA result before v_max_f32 (16 of 24 v_max per key tile were those copies). Consequence (the whole file is built
# this way): a NaN in q / k / v gives undefined attention output (it may be hidden by the max tree or skip the deferred
# rescale) instead of propagating visibly; the Whisper / HuBERT inputs are finite by construction (log-mel, LayerNorm).
build/attention.o: CXXFLAGS += -fno-honor-nans

# kernels whose hand-counted vmcnt waits (and residency) assume no scratch and a register budget: checked at build time
build/res_proj.o build/gate_ws.o: build/%.o: $(SRC_DIR)/%.hip $(wildcard $(SRC_DIR)/*.h) include/svc_hip.h
	@mkdir -p build
	$(HIPCC) $(CXXFLAGS) -c $< -o $@ -Rpass-analysis=kernel-resource-usage 2> build/$*.res || { cat build/$*.res; rm -f $@; exit 1; }
	@python3 tools/check_kernel_resources.py build/$*.res $(if $(filter res_proj,$*),'res_proj_kernelILb.ELi.ELb.ELi0E' 104,gate_ws 256) || { rm -f $@; exit 1; }
	@$(if $(filter res_proj,$*),python3 tools/check_kernel_resources.py build/$*.res 'res_proj_(ws_)?kernel' 256 || { rm -f $@; exit 1; })

# the direct DFT keeps 2 bins x 8 frames of f64 sums per thread (64 registers) and one workgroup of 160 KiB of LDS per
# CU: a spill would put its inner loop on scratch
build/mel_keyshift.o: build/%.o: $(SRC_DIR)/%.hip $(wildcard $(SRC_DIR)/*.h) include/svc_hip.h
	@mkdir -p build
	$(HIPCC) $(CXXFLAGS) -c $< -o $@ -Rpass-analysis=kernel-resource-usage 2> build/$*.res || { cat build/$*.res; rm -f $@; exit 1; }
	@python3 tools/check_kernel_resources.py build/$*.res mel_keyshift_kernel 256 || { rm -f $@; exit 1; }

# the loudness stage streams f64 sqrt / pow / division over every sample: a spill would put scratch traffic beside it
build/loudness.o: build/%.o: $(SRC_DIR)/%.hip $(wildcard $(SRC_DIR)/*.h) include/svc_hip.h
	@mkdir -p build
	$(HIPCC) $(CXXFLAGS) -c $< -o $@ -Rpass-analysis=kernel-resource-usage 2> build/$*.res || { cat build/$*.res; rm -f $@; exit 1; }
	@python3 tools/check_kernel_resources.py build/$*.res 'loudness_(power|apply)_kernel' 128 || { rm -f $@; exit 1; }

# the join of long-form conversion: stitch_seams runs a song's seams on one workgroup of up to 1024 threads (128
# registers each) with two f64 sums per candidate; a spill would put its inner loop on scratch
build/stitch.o: build/%.o: $(SRC_DIR)/%.hip $(wildcard $(SRC_DIR)/*.h) include/svc_hip.h
	@mkdir -p build
	$(HIPCC) $(CXXFLAGS) -c $< -o $@ -Rpass-analysis=kernel-resource-usage 2> build/$*.res || { cat build/$*.res; rm -f $@; exit 1; }
	@python3 tools/check_kernel_resources.py build/$*.res 'stitch_(seams|write)_kernel' 128 || { rm -f $@; exit 1; }

# feature retrieval: knn_topk keeps 64 accumulator and 32 top-k registers per lane and indexes both statically; a spill
# would put the selection epilogue on scratch
build/retrieve.o: build/%.o: $(SRC_DIR)/%.hip $(wildcard $(SRC_DIR)/*.h) include/svc_hip.h
	@mkdir -p build
	$(HIPCC) $(CXXFLAGS) -c $< -o $@ -Rpass-analysis=kernel-resource-usage 2> build/$*.res || { cat build/$*.res; rm -f $@; exit 1; }
	@python3 tools/check_kernel_resources.py build/$*.res '(knn_topk|retrieve_blend|index_norms)_kernel' 256 || { rm -f $@; exit 1; }

# index compaction: index_sum keeps a row's 32 int64 column sums per lane (64 registers) under two rows of loads in
# flight; a spill would put the streaming loop on scratch
build/index_kmeans.o: build/%.o: $(SRC_DIR)/%.hip $(wildcard $(SRC_DIR)/*.h) include/svc_hip.h
	@mkdir -p build
	$(HIPCC) $(CXXFLAGS) -c $< -o $@ -Rpass-analysis=kernel-resource-usage 2> build/$*.res || { cat build/$*.res; rm -f $@; exit 1; }
	@python3 tools/check_kernel_resources.py build/$*.res '(index_\w+|inertia_\w+)_kernel' 128 || { rm -f $@; exit 1; }

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(OBJS) -o $@

# Device assembly of every kernel file, with the object rule's flags (per-file additions included). A device-code
# refactor is proved by `make isa` in the parent tree and in the new one, then tools/isa_diff.py on the two build/isa.
ISA := $(patsubst $(SRC_DIR)/%.hip,build/isa/%.s,$(SRCS))

isa: $(ISA)

build/isa/%.s: $(SRC_DIR)/%.hip $(wildcard $(SRC_DIR)/*.h) include/svc_hip.h
	@mkdir -p build/isa
	$(HIPCC) $(CXXFLAGS) --cuda-device-only -S -Wno-unused-command-line-argument $< -o $@

build/isa/attention.s: CXXFLAGS += -fno-honor-nans

clean:
	rm -rf build $(LIB)

.PHONY: all clean isa
