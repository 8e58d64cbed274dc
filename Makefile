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

HIPFLAGS  := -std=c++17 -O3 -fPIC -fvisibility=hidden -fvisibility-inlines-hidden -Iinclude --offload-arch=$(ARCH) -fno-slp-vectorize -mllvm -amdgpu-kernarg-preload-count=16
HOSTFLAGS := -std=c++17 -O3 -fPIC -fvisibility=hidden -fvisibility-inlines-hidden -Iinclude -ffp-contract=off -D__HIP_PLATFORM_AMD__

# the units of each library, in link order, and the headers that all units of a kind depend on
HIP_UNITS   := jsg_kernels jsg_stft_a jsg_stft_b jsg_filterbank jsg_display_axis jsg_cstft jsg_pvoc jsg_hpss jsg_resample jsg_cqt jsg_yin jsg_rhythm jsg_cepstral jsg_spectral
HOST_UNITS  := jsg_engine jsg_host_math jsg_filterbank_host jsg_display_axis_host jsg_cqt_host jsg_yin_host jsg_rhythm_host jsg_cepstral_host jsg_spectral_host
XHIP_UNITS  := jsgx_beat jsgx_cdist jsgx_dtw jsgx_viterbi jsgx_pyin jsgx_knn jsgx_rqa jsgx_path_enhance jsgx_nmf jsgx_pcen jsgx_peak jsgx_sync jsgx_agglo
XHOST_UNITS := jsgx_beat_host jsgx_dtw_host jsgx_viterbi_host jsgx_pyin_host jsgx_knn_host jsgx_rqa_host jsgx_path_enhance_host jsgx_nmf_host jsgx_pcen_host jsgx_peak_host jsgx_sync_host jsgx_agglo_host
# jsg_spans.h and jsg_launch.h have no state; they are all that the two libraries share
SHARED := $(SRC)/jsg_spans.h $(SRC)/jsg_launch.h
KDEPS  := $(SRC)/jsg_stft_kernel.h $(SRC)/jsg_runs_grid.h $(SRC)/jsg_internal.h $(SRC)/jsg_exact_math.h $(SHARED) include/jsg.h
HDEPS  := $(SRC)/jsg_internal.h $(SRC)/jsg_block_queue.h $(SRC)/jsg_exact_math.h $(SRC)/jsg_colormap_tables.inc $(SHARED) include/jsg.h
XDEPS  := $(SRC)/jsgx_internal.h $(SRC)/jsgx_cost_tile.h $(SRC)/jsgx_plane_tiles.h $(SRC)/jsgx_segments.h $(SHARED) include/jsgx.h

$(HIP_UNITS:%=$(OBJ)/%.o): $(KDEPS)
$(HOST_UNITS:%=$(OBJ)/%.o): $(HDEPS)
$(XHIP_UNITS:%=$(OBJ)/%.o) $(XHOST_UNITS:%=$(OBJ)/%.o): $(XDEPS)
# the 512 / 1024 / 2048 / 8192-point kernels: ILP-first machine scheduler (see the unit's header comment)
$(OBJ)/jsg_stft_a.o: UNITFLAGS := -mllvm -amdgpu-sched-strategy=max-ilp

$(HIP_UNITS:%=$(OBJ)/%.o) $(XHIP_UNITS:%=$(OBJ)/%.o): $(OBJ)/%.o: $(SRC)/%.hip
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(UNITFLAGS) -c $< -o $@
$(HOST_UNITS:%=$(OBJ)/%.o) $(XHOST_UNITS:%=$(OBJ)/%.o): $(OBJ)/%.o: $(SRC)/%.cpp
	@mkdir -p $(OBJ)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@

$(OUT): $(HIP_UNITS:%=$(OBJ)/%.o) $(HOST_UNITS:%=$(OBJ)/%.o)
$(OUTX): $(XHIP_UNITS:%=$(OBJ)/%.o) $(XHOST_UNITS:%=$(OBJ)/%.o)
$(OUT) $(OUTX):
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $^

oracle:
	$(MAKE) -C oracle port ref

test-cpp: lib
	g++ -std=c++17 -O1 -Wall -Wextra -Iinclude tests/cpp/host_dropin_test.cpp -o $(OBJ)/host_dropin_test \
	    -Ljadespectrogram_amd -ljsg -Wl,-rpath,$(CURDIR)/jadespectrogram_amd

clean:
	rm -rf $(OBJ) $(OUT) $(OUTX)
