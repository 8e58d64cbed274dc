// Test driver for the display frequency axis of the C++ drop-in (jadespectrogram_amd/host/Spectrogram.h): a plugin that draws a log
// axis at its window's pixel height.  Feeds a tone, switches the display to LOG 20 Hz .. 20 kHz at `height` rows, draws one image and
// prints the geometry and the row of the brightest pixel as JSON for tests/test_gpu_freq_axis.py.
//   usage: display_axis_test <height> <fftsize> <tone_hz>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../jadespectrogram_amd/host/Spectrogram.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int height = atoi(argv[1]), fftsize = atoi(argv[2]);
    const double tone = atof(argv[3]);
    Spectrogram spec;
    spec.preparetoProcess(1, fftsize);
    spec.setSamplerate(48000.f);
    spec.setmemoryTime_s(0.5f);
    spec.setFFTSize(size_t(fftsize));
    SpectrogramGpuDisplay display(spec, 256, CColorPalette::kBW);
    if (display.height() != fftsize / 2 + 1) return 4;
    if (display.setFrequencyAxis(JSG_AXIS_LOG, height, 0.f, 20000.f) != JSG_ERR_INVALID) return 5;   // LOG needs fmin > 0
    if (display.setFrequencyAxis(JSG_AXIS_LOG, height, 20.f, 20000.f) != JSG_OK) return 6;
    const std::vector<float> centres = display.centres();
    if (int(centres.size()) != display.height()) return 7;

    juce::MidiBuffer midi;
    long t = 0;
    for (int b = 0; b < 8; ++b) {
        juce::AudioBuffer<float> buf(1, fftsize);
        for (int i = 0; i < fftsize; ++i, ++t) buf.getWritePointer(0)[i] = float(0.5 * std::sin(2.0 * M_PI * tone * double(t) / 48000.0));
        spec.processBlock(buf, midi);
    }
    const int W = spec.getMemorySize(), H = display.height();
    std::vector<uint32_t> img(size_t(W) * size_t(H));
    int newVals = 0, pos = 0;
    if (display.update(-90.f, 40.f, img.data(), W, newVals, pos) != JSG_OK) return 8;
    // brightest rows of the newest column (black-white palette: the grey level rises with the index); the middle of that run,
    // 0 = bottom row
    const int x = (W - 1);
    uint32_t best_v = 0;
    for (int y = 0; y < H; ++y) best_v = std::max(best_v, img[size_t(y) * size_t(W) + size_t(x)] & 0xFFu);
    int top = -1, bottom = -1;
    for (int y = 0; y < H; ++y)
        if ((img[size_t(y) * size_t(W) + size_t(x)] & 0xFFu) == best_v) {
            if (top < 0) top = y;
            bottom = y;
        }
    const int row = H - 1 - (top + bottom) / 2;
    printf("{\"W\": %d, \"H\": %d, \"centre_lo\": %.6f, \"centre_hi\": %.6f, \"tone_row\": %d, \"tone_row_hz\": %.6f}\n", W, H,
           double(centres.front()), double(centres.back()), row, double(centres[size_t(row)]));
    return 0;
}
