// Second launch of the luma-domain NV12 transcode (fsr1_transcode_luma): RCAS on the Y plane and the bilinear resample of the CbCr plane
// in ONE grid of two-wave workgroups, no LDS, no barrier.
//   * the first tiles_x * tiles_y * frames workgroups are the strips of fsr1_rcas_mono.hip (rcas_mono_tile, fsr1_rcas_mono_kernel.h) on
//     the uint8 intermediary -> the Y plane: the same code in the same workgroup order, so the Y bytes are those rcas_mono_kernel stores;
//   * the workgroups behind them are chroma strips.  They read `in` only, so nothing orders them against the RCAS strips; they fill the
//     tail of a launch that is paced by its row streams and has VALU to spare.
// The chroma strip ("THE PINNED LUMA-DOMAIN TRANSCODE", fsr1_hip.h):
//   * a wave owns 64 x 4 adjacent output pairs and walks a strip of output pair rows; a lane owns four adjacent pairs: 8 bytes, one
//     store a row where the host found every such address aligned (out_wide), 16-bit pair stores otherwise and in the lane the plane's
//     right edge cuts;
//   * horizontally, k0, k0 + 1 (clamped to the plane: indices, never addresses past it) and f of a lane's four columns are computed once
//     per strip.  The pairs a lane needs from an input row are a contiguous run; where the rows start on dwords and the run fits three of
//     them (in_wide: every upscale of an aligned surface — the host has walked the columns with the device's own arithmetic) it is
//     loaded as three aligned dwords and the eight taps are selected from registers; otherwise (minification, 2-byte-aligned rows) each
//     tap is its own 16-bit load;
//   * vertically, j0 never decreases down a strip: the two horizontally blended input rows h(j0), h(j0 + 1) live in registers as
//     binary32 (16 VGPRs) and an input row is blended only when a row the strip does not hold is asked for — at 2x once per strip for
//     two output rows; under minification j0 advances by more than one and both are replaced.  A blended row is a function of its
//     index alone, so holding it changes no bit;
//   * every product, sum and difference is rounded to binary32 by itself (__fmul_rn / __fadd_rn / __fsub_rn: never contracted).
#include <algorithm>
#include <cmath>

#include "fsr1_rcas_mono_kernel.h"

namespace fsr1 {

constexpr int kChromaCols = 4;  // output pairs a lane owns
constexpr int kChromaWaveCols = 64 * kChromaCols;

// h(j): the input pair row at `row` blended horizontally at a lane's four columns -> hb (Cb), hr (Cr).  ka / kb: the clamped indices of
// the two taps of each column, f: its weight; d0 / dmax: the dword of the row the lane's run starts in, and the row's last.
template <bool IN_WIDE>
__device__ __forceinline__ void chroma420_blend_row(const char* row, const int (&ka)[kChromaCols], const int (&kb)[kChromaCols], const float (&f)[kChromaCols],
                                                    int d0, int dmax, float (&hb)[kChromaCols], float (&hr)[kChromaCols]) {
  uint32_t w0 = 0u, w1 = 0u, w2 = 0u;
  if constexpr (IN_WIDE) {
    const uint32_t* const w = reinterpret_cast<const uint32_t*>(row);
    w0 = w[d0], w1 = w[min(d0 + 1, dmax)], w2 = w[min(d0 + 2, dmax)];
  }
#pragma unroll
  for (int i = 0; i < kChromaCols; ++i) {
    uint32_t pa, pb;
    if constexpr (IN_WIDE) {
      const int oa = (ka[i] >> 1) - d0, ob = (kb[i] >> 1) - d0;
      const uint32_t da = oa == 0 ? w0 : (oa == 1 ? w1 : w2), db = ob == 0 ? w0 : (ob == 1 ? w1 : w2);
      pa = (ka[i] & 1) ? da >> 16 : da & 0xffffu;
      pb = (kb[i] & 1) ? db >> 16 : db & 0xffffu;
    } else {
      const uint16_t* const p = reinterpret_cast<const uint16_t*>(row);
      pa = p[ka[i]], pb = p[kb[i]];
    }
    const float a_cb = (float)(pa & 0xffu), a_cr = (float)(pa >> 8), b_cb = (float)(pb & 0xffu), b_cr = (float)(pb >> 8);
    hb[i] = __fadd_rn(a_cb, __fmul_rn(f[i], __fsub_rn(b_cb, a_cb)));
    hr[i] = __fadd_rn(a_cr, __fmul_rn(f[i], __fsub_rn(b_cr, a_cr)));
  }
}

template <bool IN_WIDE, bool OUT_WIDE>
__device__ __forceinline__ void chroma420_strip(const Chroma420Args& c, int frame, int x0, int y0, int lane, bool stream) {
  constexpr int G = kChromaCols;
  const int K0 = x0 + G * lane;
  int ka[G], kb[G];
  float f[G];
#pragma unroll
  for (int i = 0; i < G; ++i) {
    const float u = __fadd_rn(__fmul_rn((float)(K0 + i), c.scale_x), c.off_x), fl = floorf(u);
    const int k0 = (int)fminf(fl, (float)c.cw);  // (lanes right of the plane: far beyond it, clamped like every other index)
    f[i] = __fsub_rn(u, fl);
    ka[i] = min(max(k0, 0), c.cw - 1);
    kb[i] = min(max(k0 + 1, 0), c.cw - 1);
  }
  const char* const in_frame = c.in + (long long)frame * c.in_frame_stride;
  char* const out_frame = c.out + (long long)frame * c.out_frame_stride;
  const int d0 = ka[0] >> 1, dmax = (c.cw - 1) >> 1;  // dwords of a row: the lane's first, the row's last

  auto code = [](float v) { return (uint32_t)__fadd_rn(fminf(fmaxf(v, 0.0f), 255.0f), 0.5f); };

  float h0b[G] = {}, h0r[G] = {}, h1b[G] = {}, h1r[G] = {};  // h(ia), h(ib): Cb and Cr of the lane's four columns
  int ia = -1, ib = -1;                                        // the input rows they hold
#pragma unroll 1
  for (int r = 0; r < c.rows; ++r) {
    const int J = y0 + r;  // wave-uniform, like everything vertical
    if (J >= c.CH) break;
    const float v = __fadd_rn(__fmul_rn((float)J, c.scale_y), c.off_y), fl = floorf(v), g = __fsub_rn(v, fl);
    const int j0 = (int)fminf(fl, (float)c.ch);
    const int ja = min(max(j0, 0), c.ch - 1), jb = min(max(j0 + 1, 0), c.ch - 1);
    if (ja != ia) {
      if (ja == ib) {
#pragma unroll
        for (int i = 0; i < G; ++i) h0b[i] = h1b[i], h0r[i] = h1r[i];
      } else {
        chroma420_blend_row<IN_WIDE>(in_frame + (long long)ja * c.in_pitch, ka, kb, f, d0, dmax, h0b, h0r);
      }
      ia = ja;
    }
    if (jb != ib) {
      if (jb == ia) {
#pragma unroll
        for (int i = 0; i < G; ++i) h1b[i] = h0b[i], h1r[i] = h0r[i];
      } else {
        chroma420_blend_row<IN_WIDE>(in_frame + (long long)jb * c.in_pitch, ka, kb, f, d0, dmax, h1b, h1r);
      }
      ib = jb;
    }
    uint32_t pair[G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const uint32_t cb = code(__fadd_rn(h0b[i], __fmul_rn(g, __fsub_rn(h1b[i], h0b[i]))));
      const uint32_t cr = code(__fadd_rn(h0r[i], __fmul_rn(g, __fsub_rn(h1r[i], h0r[i]))));
      pair[i] = cb | (cr << 8);
    }
    char* const dst = out_frame + (long long)J * c.out_pitch + (size_t)(uint32_t)K0 * 2u;
    if (OUT_WIDE && K0 + G <= c.CW) {
      store_out<8>(dst, Words<2>::T{pair[0] | (pair[1] << 16), pair[2] | (pair[3] << 16)}, stream);
    } else {
#pragma unroll
      for (int i = 0; i < G; ++i)
        if (K0 + i < c.CW) store_out<2>(dst + 2 * i, (uint16_t)pair[i], stream);
    }
  }
}

// RCAS strips first, in rcas_mono_kernel's own order; chroma strips behind them (their ids start wherever the RCAS strips end, so the
// XCD a chroma id lands on is not the one xcd_swizzle assumes: it is a permutation of the strips either way, and neighbouring chroma
// strips share at most two input rows).
template <bool EXACT, bool OPTS, bool WIDE>
__global__ void __launch_bounds__(kRcasMonoThreads) rcas_luma_kernel(const RcasArgs a, const Chroma420Args c) {
  constexpr int FMT = FSR1_FORMAT_R8_UNORM;
  const int rcas_groups = a.tiles_x * a.tiles_y * a.frames;
  const int b = (int)blockIdx.x;
  if (b < rcas_groups) {
    rcas_mono_tile<FMT, EXACT, OPTS, WIDE, kRcasMonoRing, kRcasMonoCols<FMT>>(a, xcd_swizzle(b, rcas_groups, a.xcd_shift));
    return;
  }
  const int tiles_per_frame = c.tiles_x * c.tiles_y;
  const int t = xcd_swizzle(b - rcas_groups, tiles_per_frame * a.frames, a.xcd_shift);
  const int frame = t / tiles_per_frame;
  const int tf = t - frame * tiles_per_frame;
  const int ty = tf / c.tiles_x, tx = tf - ty * c.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = (tx * kRcasMonoWaves + wave) * kChromaWaveCols, y0 = ty * c.rows;
  if (x0 >= c.CW) return;  // whole wave outside
  const bool stream = (a.flags & FSR1_FLAG_OUTPUT_STREAMING) != 0;
  if (c.in_wide && c.out_wide) chroma420_strip<true, true>(c, frame, x0, y0, lane, stream);
  else if (c.in_wide) chroma420_strip<true, false>(c, frame, x0, y0, lane, stream);
  else if (c.out_wide) chroma420_strip<false, true>(c, frame, x0, y0, lane, stream);
  else chroma420_strip<false, false>(c, frame, x0, y0, lane, stream);
}

// Chroma strips: 8 output pair rows — the height of a 4K frame's RCAS strips, which at 2x blends five or six input rows for eight stored
// ones — by two waves of 256 pairs.  (Unmeasured against other heights: the strips are a tenth of the launch's workgroups.)
void chroma420_geometry(int CW, int CH, int* tiles_x, int* tiles_y, int* rows) {
  *rows = 8;
  *tiles_x = (CW + kChromaWaveCols * kRcasMonoWaves - 1) / (kChromaWaveCols * kRcasMonoWaves);
  *tiles_y = (CH + *rows - 1) / *rows;
}

// Dwords the run of input pairs of one lane spans at most (3: what in_wide loads), found with the device's own arithmetic over every lane
// of the plane's width: clamp(k0) of its first column to clamp(k0 + 1) of its last.
int chroma420_run_dwords(int CW, int cw, float scale_x, float off_x) {
  auto k0 = [&](int K) {
    const float p = (float)K * scale_x;  // two roundings, as on the device (the unit is built with -ffp-contract=off)
    return (int)std::fmin(std::floor(p + off_x), (float)cw);
  };
  int worst = 1;
  for (int K = 0; K < CW; K += kChromaCols) {
    const int first = std::min(std::max(k0(K), 0), cw - 1), last = std::min(std::max(k0(K + kChromaCols - 1) + 1, 0), cw - 1);
    worst = std::max(worst, (last >> 1) - (first >> 1) + 1);
  }
  return worst;
}

// wide: the RCAS groups move as one access (rcas_mono_launch's rule).  chroma_only: no RCAS strips — the chroma resample as a launch of its
// own, which only the measurement build of fsr1_transcode_luma asks for.
hipError_t rcas_luma_launch(const RcasArgs& a, const Chroma420Args& c, bool exact, bool wide, bool chroma_only, hipStream_t stream) {
  RcasArgs r = a;
  if (chroma_only) r.tiles_y = 0;
  const dim3 grid((unsigned)((r.tiles_x * r.tiles_y + c.tiles_x * c.tiles_y) * r.frames)), block(kRcasMonoThreads);
  const bool opts = (a.flags & (FSR1_FLAG_RCAS_DENOISE | FSR1_FLAG_HDR_SQUARE)) != 0;
#define FSR1_RCASL_W(E, O) do { if (wide) hipLaunchKernelGGL((rcas_luma_kernel<E, O, true>), grid, block, 0, stream, r, c); \
                                else hipLaunchKernelGGL((rcas_luma_kernel<E, O, false>), grid, block, 0, stream, r, c); } while (0)
#define FSR1_RCASL_O(E) do { if (opts) FSR1_RCASL_W(E, true); else FSR1_RCASL_W(E, false); } while (0)
  if (exact) FSR1_RCASL_O(true);
  else FSR1_RCASL_O(false);
#undef FSR1_RCASL_O
#undef FSR1_RCASL_W
  return hipGetLastError();
}

}  // namespace fsr1
