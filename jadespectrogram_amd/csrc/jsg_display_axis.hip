// libjsg.so, display frequency axes: the colour kernel over a row table and its launcher (jsg_colormap_axis_launch; include/jsg.h,
// section 2c).  The row table and its tiles come from jsg_display_axis_host.cpp.
//
//   colormap_axis_kernel  dB ring columns -> `height` ARGB image rows on a linear / log / mel axis.  A workgroup takes 64 columns and
//                one row tile (at most 64 consecutive rows whose bins lie in one span of at most kAxisSpan bins, cut on the host):
//                  stage   each wave loads 16 columns of the span, lanes along the bins (coalesced), into LDS [column][bin];
//                  reduce  lane = column, each wave walks its rows (wave-uniform bounds: no divergence), the max of the row's bins
//                          or the interpolation between two bins, read across the columns with a row stride of kAxisSpan + 1 dwords
//                          (64 different banks);
//                  write   lane = column again: the rows go out as coalesced non-temporal stores, no second transpose.
//                A tile that is one row wider than kAxisSpan bins walks its span in steps of kAxisSpan, keeping the running maximum in
//                registers.  Each dB value is staged about once whatever the axis; 33 KB of LDS per workgroup + the 4 KB palette.
#include "jsg_stft_kernel.h"

namespace jsg {

struct AxisKArgs {
    const float* db;
    long long db_pitch;
    int ring_w, col_first, n_cols, x_first, x_wrap;
    int height;                  // image rows
    const int* rows;             // first_bin[height], n_bins[height], interp_t[height] (float bits)
    const int* tiles;            // (first row, rows, first bin, bins) per tile
    const int* lut;
    int n_colors;
    float vmin, vmax, top, mult;
    unsigned* argb;
    long long argb_pitch;
    unsigned char* index;
    long long index_pitch;
};

constexpr int AX_COLS = 64;                       // columns per workgroup (one per lane)
constexpr int AX_RPW = kAxisTileRows / 4;         // rows per wave

__global__ __launch_bounds__(256) void colormap_axis_kernel(const AxisKArgs a) {
#pragma clang fp contract(off)
    __shared__ float s_db[AX_COLS][kAxisSpan + 1];
    __shared__ int s_lut[1024];
    __shared__ int s_row[3][kAxisTileRows];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int* tile = a.tiles + 4 * blockIdx.y;
    const int row0 = tile[0], n_rows = tile[1], bin_lo = tile[2], span = tile[3];
    const int col0 = blockIdx.x * AX_COLS;
    const bool lut_in_lds = a.n_colors <= 1024;

    if (tid < n_rows) {
        s_row[0][tid] = a.rows[row0 + tid];
        s_row[1][tid] = a.rows[a.height + row0 + tid];
        s_row[2][tid] = a.rows[2 * a.height + row0 + tid];
    }
    if (lut_in_lds)
        for (int k = tid; k < a.n_colors; k += 256) s_lut[k] = a.lut[k];
    float acc[AX_RPW];
#pragma unroll
    for (int q = 0; q < AX_RPW; ++q) acc[q] = -__builtin_inff();

    for (int c0 = 0; c0 < span; c0 += kAxisSpan) {   // one step unless the tile is a single row wider than kAxisSpan bins
        const int cnt = min(span - c0, kAxisSpan);
        if (c0 > 0) __syncthreads();                   // the previous step has been reduced
        // stage: wave takes columns wave + 4q, lanes run along the bins; all loads before the first LDS store.  The 16 column
        // addresses are formed anew in every step: the empty asm hides the ring geometry from loop-invariant code motion, which
        // would otherwise keep column pointers live across the step loop and the reduction (SGPR spills; tools/kernel_regs.py)
        int col_first = a.col_first;
        long long db_pitch = a.db_pitch;
        asm volatile("" : "+s"(col_first), "+s"(db_pitch));
        float v[AX_COLS / 4][2];
        const int halves = cnt > 64 ? 2 : 1;
        // Loads without masks: a column past n_cols reads the last column, a bin past the step's end reads its last bin.  Those
        // LDS entries are never used (the reduction reads bins < cnt, the write phase skips columns >= n_cols).
        const int b0 = min(lane, cnt - 1), b1 = min(lane + 64, cnt - 1);
#pragma unroll
        for (int q = 0; q < AX_COLS / 4; ++q) {
            const int i = min(col0 + wave + 4 * q, a.n_cols - 1);
            int col = col_first + i;                   // col_first < ring_w and i < n_cols <= ring_w
            if (col >= a.ring_w) col -= a.ring_w;
            const float* src = a.db + (long long)col * db_pitch + bin_lo + c0;
            v[q][0] = src[b0];
            v[q][1] = halves > 1 ? src[b1] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < AX_COLS / 4; ++q)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (h < halves) s_db[wave + 4 * q][lane + 64 * h] = v[q][h];
        __syncthreads();
        // reduce: lane = column, rows wave + 4q of the tile
        const int lo = bin_lo + c0;
#pragma unroll
        for (int q = 0; q < AX_RPW; ++q) {
            const int r = wave + 4 * q;
            if (r >= n_rows) break;
            const int first = s_row[0][r], nb = s_row[1][r];
            if (nb > 0) {
                const int j0 = max(first, lo) - lo, j1 = min(first + nb, lo + cnt) - lo;
                float m = acc[q];
                for (int j = j0; j < j1; ++j) {
                    const float x = s_db[lane][j];
                    m = (x > m || x != x) ? x : m;     // a NaN sticks (v_max_f32 would drop it)
                }
                acc[q] = m;
            } else if (first >= lo && first + 1 < lo + cnt) {
                const float t = __int_as_float(s_row[2][r]);
                const float x0 = s_db[lane][first - lo], x1 = s_db[lane][first + 1 - lo];
                const float d = x1 - x0;               // three roundings (fp contract off above)
                const float p = t * d;
                acc[q] = x0 + p;
            }
        }
    }
    // write: lane = column; image row height-1-row (low frequencies at the bottom)
    const int i = col0 + lane;
    if (i < a.n_cols) {
        const int x = (a.x_first + i) % a.x_wrap;       // x_first < x_wrap; wraps at most once when n_cols <= x_wrap
#pragma unroll
        for (int q = 0; q < AX_RPW; ++q) {
            const int r = wave + 4 * q;
            if (r >= n_rows) break;
            const int idx = color_index(acc[q], a.vmin, a.vmax, a.top, a.mult, a.n_colors);
            const long long y = a.height - 1 - (row0 + r);
            if (a.argb) {
                const int rgb = lut_in_lds ? s_lut[idx] : a.lut[idx];
                __builtin_nontemporal_store((unsigned)rgb | 0xFF000000u, &a.argb[y * a.argb_pitch + x]);
            }
            if (a.index) a.index[y * a.index_pitch + x] = (unsigned char)idx;
        }
    }
}

// load the unit's code object now (jsg_freq_axis_create), not inside the first display tick
void touch_axis_module() { (void)preload_code_object(reinterpret_cast<const void*>(&colormap_axis_kernel)); }

}  // namespace jsg

using namespace jsg;

extern "C" {

int jsg_colormap_axis_launch(const jsg_colormap_args* g, const jsg_freq_axis* ax, void* stream) {
    if (!g || !ax) return jsg_fail(JSG_ERR_INVALID, "jsg_colormap_axis_launch: null argument");
    if (g->n_cols == 0) return JSG_OK;
    if (!g->db || !g->lut || g->height <= 0 || g->ring_width <= 0 || g->n_cols < 0 || g->x_wrap <= 0 || g->n_colors <= 0 ||
        g->col_first < 0 || g->x_first < 0 || (!g->argb_out && !g->index_out))
        return jsg_fail(JSG_ERR_INVALID, "jsg_colormap_axis_launch: bad geometry");
    if (g->n_cols > g->ring_width) return jsg_fail(JSG_ERR_INVALID, "jsg_colormap_axis_launch: more columns than the ring holds");
    if (g->index_out && g->n_colors > 256)
        return jsg_fail(JSG_ERR_INVALID, "jsg_colormap_axis_launch: the 8-bit index plane needs n_colors <= 256");
    if ((g->argb_out && g->argb_pitch < g->x_wrap) || (g->index_out && g->index_pitch < g->x_wrap))
        return jsg_fail(JSG_ERR_INVALID, "jsg_colormap_axis_launch: image pitch smaller than x_wrap (rows would overlap / leave the image)");
    if (g->n_colors > 65535) return jsg_fail(JSG_ERR_UNSUPPORTED, "jsg_colormap_axis_launch: n_colors > 65535");
    if (g->height != ax->n / 2 + 1)
        return jsg_fail(JSG_ERR_INVALID, "jsg_colormap_axis_launch: the axis was built for another FFT size (height must be n/2+1)");
    if (g->db_pitch < g->height) return jsg_fail(JSG_ERR_INVALID, "jsg_colormap_axis_launch: db_pitch smaller than n/2+1");
    const DeviceBlob::Where at = ax->blob.where();
    if (at == DeviceBlob::kNoDevice) return jsg_fail(JSG_ERR_NO_DEVICE, "jsg_colormap_axis_launch: no device");
    if (at != DeviceBlob::kHere) return jsg_fail(JSG_ERR_INVALID, "jsg_colormap_axis_launch: the axis was created on another device");
    AxisKArgs ka{};
    ka.db = g->db;
    ka.db_pitch = g->db_pitch;
    ka.ring_w = g->ring_width;
    ka.col_first = g->col_first % g->ring_width;
    ka.n_cols = g->n_cols;
    ka.x_first = g->x_first % g->x_wrap;
    ka.x_wrap = g->x_wrap;
    ka.height = ax->height;
    ka.rows = ax->d_rows;
    ka.tiles = ax->d_tiles;
    ka.lut = g->lut;
    ka.n_colors = g->n_colors;
    ka.vmin = g->vmin;
    ka.vmax = g->vmax;
    ka.top = g->vmax * 0.9999f;
    ka.mult = g->access_mult;
    ka.argb = g->argb_out;
    ka.argb_pitch = g->argb_pitch;
    ka.index = g->index_out;
    ka.index_pitch = g->index_pitch;
    dim3 grid((g->n_cols + AX_COLS - 1) / AX_COLS, ax->n_tiles);
    hipLaunchKernelGGL(colormap_axis_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), ka);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return jsg_fail_hip(err, "jsg_colormap_axis_launch");
    return JSG_OK;
}

}  // extern "C"
