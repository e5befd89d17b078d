# Build everything in-tree (the .so files travel to the GPU box with the snapshot).
#   make            libsdr_amd.so (HIP kernels + C ABI, gfx950), libsdr_host.so (the reference's
#                   C++ stage/primitive API over the C ABI), bin/sdr_project (the receiver CLI),
#                   bin/sdr_multi (the multi-channel receiver),
#                   oracle/liboracle.so (+ oracle/_ref when the reference tree is present here)
HIPCC    ?= /opt/rocm/bin/hipcc
CXX      ?= g++
ROCM     ?= /opt/rocm
ARCH     ?= gfx950
PKG      := real-time-sdr_amd
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-gpu-flush-denormals-to-zero \
            -mllvm -pragma-unroll-threshold=1000000 \
            -Wall -Iinclude
LIB      := $(PKG)/libsdr_amd.so
SRCS     := $(PKG)/csrc/sdr_kernels.hip $(PKG)/csrc/sdr_ctx.hip $(PKG)/csrc/sdr_plls.cpp $(PKG)/csrc/sdr_streams.hip \
            $(PKG)/csrc/sdr_primitives.hip $(PKG)/csrc/sdr_frontend.hip $(PKG)/csrc/sdr_pll.hip $(PKG)/csrc/sdr_scan.hip \
            $(PKG)/csrc/sdr_meter.hip $(PKG)/csrc/sdr_audio.hip $(PKG)/csrc/sdr_split.hip \
            $(PKG)/csrc/sdr_rds.hip $(PKG)/csrc/sdr_rds_track.hip $(PKG)/csrc/sdr_rds_carrier.hip \
            $(PKG)/csrc/sdr_taps.cpp $(PKG)/csrc/sdr_rds_text.cpp
OBJS     := $(patsubst $(PKG)/csrc/%,build/%.o,$(SRCS))
HDRS     := include/sdr_amd.h $(PKG)/csrc/pll_math.h $(PKG)/csrc/sdr_internal.h $(PKG)/csrc/demod_phase.h \
            $(PKG)/csrc/nco.h $(PKG)/csrc/stage_device.h $(PKG)/csrc/stage_host.h

# host C++ (no device code): compiled by the system g++ against the HIP runtime headers
HOSTFLAGS := -O2 -std=c++17 -fPIC -Wall -Wextra -pthread -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include \
             -Iinclude -Iinclude/dropin -I$(PKG)/host
HOSTLIB   := $(PKG)/libsdr_host.so
HOSTSRCS  := $(PKG)/host/dropin_primitives.cpp $(PKG)/host/dropin_stages.cpp $(PKG)/host/rds_frame.cpp \
             $(PKG)/host/sdr_multi_engine.cpp $(PKG)/host/sdr_scan_run.cpp
HOSTHDRS  := $(wildcard include/dropin/*.h) $(PKG)/host/hip_util.h $(PKG)/host/wide_split.h include/sdr_amd.h include/sdr_multi.h \
             include/sdr_multi_tuned.h include/sdr_multi_meter.h include/sdr_multi_audio.h include/sdr_scan_run.h \
             include/sdr_multi_wide.h include/sdr_wide_scan.h include/sdr_multi_rds.h include/sdr_multi_wide16.h
CLI       := $(PKG)/bin/sdr_project
MULTI     := $(PKG)/bin/sdr_multi

.PHONY: all lib host oracle clean
all: lib host oracle

lib: $(LIB)
host: $(HOSTLIB) $(CLI) $(MULTI)

# one object per translation unit (compiled in parallel), linked into the shared library
# the stage kernels keep their f32 multiply-adds scalar (packed f32 runs at half rate): no SLP;
# the lane-pair PLL step is faster scalar too (packed-f32 results cost a wait state on gfx950,
# profiles/r03/ab_pll_split3.txt)
build/sdr_kernels.hip.o: HIPFLAGS += -fno-slp-vectorize
# the units split off sdr_kernels.hip keep its flags for the kernels they took along
build/sdr_ctx.hip.o build/sdr_streams.hip.o build/sdr_primitives.hip.o: HIPFLAGS += -fno-slp-vectorize
# the band scan's complex multiply-adds are four scalar v_fma_f32 with SGPR twiddles: no SLP either
build/sdr_scan.hip.o: HIPFLAGS += -fno-slp-vectorize
# the meter's noise FIR keeps its multiplies and adds scalar and in tap order: no SLP
build/sdr_meter.hip.o: HIPFLAGS += -fno-slp-vectorize
# audio finishing: every product and sum scalar and on its own, as the model states them
build/sdr_audio.hip.o: HIPFLAGS += -fno-slp-vectorize
build/sdr_pll.hip.o: HIPFLAGS += -fno-slp-vectorize -mllvm -amdgpu-sched-strategy=max-ilp
# (the lane-pair PLL step scheduled for ILP: 212.4 -> 210.4 shader cycles per step, profiles/r04/ab_sched.txt)

build/%.o: $(PKG)/csrc/% $(HDRS) Makefile
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -fPIC -shared -Wl,-soname,libsdr_amd.so -o $@ $(OBJS)

$(HOSTLIB): $(HOSTSRCS) $(HOSTHDRS) $(LIB)
	$(CXX) $(HOSTFLAGS) -shared -o $@ $(HOSTSRCS) -L$(PKG) -lsdr_amd -L$(ROCM)/lib -lamdhip64 \
	    -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,$(ROCM)/lib

$(CLI): $(PKG)/host/sdr_project.cpp $(HOSTLIB)
	@mkdir -p $(dir $@)
	$(CXX) $(HOSTFLAGS) -o $@ $< -L$(PKG) -lsdr_host -Wl,-rpath,'$$ORIGIN/..'

$(MULTI): $(PKG)/host/sdr_multi.cpp include/sdr_multi.h include/sdr_multi_tuned.h include/sdr_multi_meter.h include/sdr_multi_audio.h include/sdr_scan_run.h include/sdr_multi_wide.h include/sdr_wide_scan.h include/sdr_multi_rds.h include/sdr_multi_wide16.h $(HOSTLIB)
	@mkdir -p $(dir $@)
	$(CXX) $(HOSTFLAGS) -o $@ $< -L$(PKG) -lsdr_host -lsdr_amd -L$(ROCM)/lib -lamdhip64 \
	    -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,$(ROCM)/lib

oracle: host
	$(MAKE) -C oracle

clean:
	rm -f $(LIB) $(HOSTLIB) $(CLI) $(MULTI)
	rm -rf build
	$(MAKE) -C oracle clean
