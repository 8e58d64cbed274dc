# Builds libjsg.so (hand-written HIP for gfx950 + C-ABI) and its companion libjsgx.so (include/jsgx.h) without Python; the same
# commands as jadespectrogram_amd/_build.py.  `make test-cpp` builds the C++ drop-in test driver against it.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
SRC   := jadespectrogram_amd/csrc
OUT   := jadespectrogram_amd/libjsg.so
OUTX  := jadespectrogram_amd/libjsgx.so
OBJ   := jadespectrogram_amd/build

.PHONY: lib oracle test-cpp clean
lib: $(OUT) $(OUTX)

HIPFLAGS := -std=c++17 -O3 -fPIC -fvisibility=hidden -fvisibility-inlines-hidden -Iinclude --offload-arch=$(ARCH) -fno-slp-vectorize -mllvm -amdgpu-kernarg-preload-count=16
KDEPS    := $(SRC)/jsg_stft_kernel.h $(SRC)/jsg_runs_grid.h $(SRC)/jsg_internal.h $(SRC)/jsg_spans.h $(SRC)/jsg_exact_math.h include/jsg.h

$(OBJ)/jsg_kernels.o: $(SRC)/jsg_kernels.hip $(KDEPS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
# the 512 / 1024 / 2048 / 8192-point kernels: ILP-first machine scheduler (see the unit's header comment)
$(OBJ)/jsg_stft_a.o: $(SRC)/jsg_stft_a.hip $(KDEPS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -mllvm -amdgpu-sched-strategy=max-ilp -c $< -o $@
$(OBJ)/jsg_stft_b.o: $(SRC)/jsg_stft_b.hip $(KDEPS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsg_filterbank.o: $(SRC)/jsg_filterbank.hip $(KDEPS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsg_display_axis.o: $(SRC)/jsg_display_axis.hip $(KDEPS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsg_cstft.o: $(SRC)/jsg_cstft.hip $(SRC)/jsg_internal.h $(SRC)/jsg_spans.h include/jsg.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsg_pvoc.o: $(SRC)/jsg_pvoc.hip $(SRC)/jsg_internal.h $(SRC)/jsg_spans.h include/jsg.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsg_hpss.o: $(SRC)/jsg_hpss.hip $(SRC)/jsg_internal.h $(SRC)/jsg_spans.h include/jsg.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsg_resample.o: $(SRC)/jsg_resample.hip $(SRC)/jsg_internal.h $(SRC)/jsg_spans.h include/jsg.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsg_cqt.o: $(SRC)/jsg_cqt.hip $(SRC)/jsg_internal.h $(SRC)/jsg_spans.h include/jsg.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsg_yin.o: $(SRC)/jsg_yin.hip $(SRC)/jsg_internal.h $(SRC)/jsg_spans.h include/jsg.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsg_rhythm.o: $(SRC)/jsg_rhythm.hip $(SRC)/jsg_internal.h $(SRC)/jsg_spans.h include/jsg.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsg_cepstral.o: $(SRC)/jsg_cepstral.hip $(SRC)/jsg_internal.h $(SRC)/jsg_spans.h include/jsg.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsg_spectral.o: $(SRC)/jsg_spectral.hip $(SRC)/jsg_internal.h $(SRC)/jsg_spans.h $(SRC)/jsg_exact_math.h include/jsg.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/%.o: $(SRC)/%.cpp $(SRC)/jsg_internal.h $(SRC)/jsg_spans.h $(SRC)/jsg_block_queue.h $(SRC)/jsg_exact_math.h $(SRC)/jsg_colormap_tables.inc include/jsg.h
	@mkdir -p $(OBJ)
	$(HIPCC) -std=c++17 -O3 -fPIC -fvisibility=hidden -fvisibility-inlines-hidden -Iinclude -ffp-contract=off -D__HIP_PLATFORM_AMD__ -c $< -o $@

$(OUT): $(OBJ)/jsg_kernels.o $(OBJ)/jsg_stft_a.o $(OBJ)/jsg_stft_b.o $(OBJ)/jsg_filterbank.o $(OBJ)/jsg_display_axis.o $(OBJ)/jsg_cstft.o $(OBJ)/jsg_pvoc.o $(OBJ)/jsg_hpss.o $(OBJ)/jsg_resample.o $(OBJ)/jsg_cqt.o $(OBJ)/jsg_yin.o $(OBJ)/jsg_rhythm.o $(OBJ)/jsg_cepstral.o $(OBJ)/jsg_spectral.o $(OBJ)/jsg_engine.o \
        $(OBJ)/jsg_host_math.o $(OBJ)/jsg_filterbank_host.o $(OBJ)/jsg_display_axis_host.o $(OBJ)/jsg_cqt_host.o $(OBJ)/jsg_yin_host.o $(OBJ)/jsg_rhythm_host.o $(OBJ)/jsg_cepstral_host.o $(OBJ)/jsg_spectral_host.o
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $^

# the companion library: its own units and headers, the same flags, nothing of libjsg.so
XDEPS := $(SRC)/jsgx_internal.h include/jsgx.h
$(OBJ)/jsgx_beat.o: $(SRC)/jsgx_beat.hip $(XDEPS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsgx_cdist.o: $(SRC)/jsgx_cdist.hip $(XDEPS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsgx_dtw.o: $(SRC)/jsgx_dtw.hip $(XDEPS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsgx_beat_host.o: $(SRC)/jsgx_beat_host.cpp $(XDEPS)
	@mkdir -p $(OBJ)
	$(HIPCC) -std=c++17 -O3 -fPIC -fvisibility=hidden -fvisibility-inlines-hidden -Iinclude -ffp-contract=off -D__HIP_PLATFORM_AMD__ -c $< -o $@
$(OBJ)/jsgx_dtw_host.o: $(SRC)/jsgx_dtw_host.cpp $(XDEPS)
	@mkdir -p $(OBJ)
	$(HIPCC) -std=c++17 -O3 -fPIC -fvisibility=hidden -fvisibility-inlines-hidden -Iinclude -ffp-contract=off -D__HIP_PLATFORM_AMD__ -c $< -o $@
$(OBJ)/jsgx_viterbi.o: $(SRC)/jsgx_viterbi.hip $(XDEPS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJ)/jsgx_viterbi_host.o: $(SRC)/jsgx_viterbi_host.cpp $(SRC)/jsg_spans.h $(XDEPS)
	@mkdir -p $(OBJ)
	$(HIPCC) -std=c++17 -O3 -fPIC -fvisibility=hidden -fvisibility-inlines-hidden -Iinclude -ffp-contract=off -D__HIP_PLATFORM_AMD__ -c $< -o $@
$(OUTX): $(OBJ)/jsgx_beat.o $(OBJ)/jsgx_cdist.o $(OBJ)/jsgx_dtw.o $(OBJ)/jsgx_viterbi.o $(OBJ)/jsgx_beat_host.o $(OBJ)/jsgx_dtw_host.o $(OBJ)/jsgx_viterbi_host.o
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $^

oracle:
	$(MAKE) -C oracle port ref

test-cpp: lib
	g++ -std=c++17 -O1 -Wall -Wextra -Iinclude tests/cpp/host_dropin_test.cpp -o $(OBJ)/host_dropin_test \
	    -Ljadespectrogram_amd -ljsg -Wl,-rpath,$(CURDIR)/jadespectrogram_amd

clean:
	rm -rf $(OBJ) $(OUT) $(OUTX)
