// EASU on packed 3-channel RGB images (FSR1_FORMAT_RGB16F / RGB32F / RGB8_UNORM): a (N,H,W,3) or channels_last tensor in, one out,
// no pad to four channels and no slice afterwards.
//
// The filter is fsr1_easu.hip's: the same 64 x 16 tiles of four waves, the same LDS records (R, G, B, luma*2 | analysis), the same
// per-pixel functions (easu_quad_row / easu_quad_pixel / easu_pixel_with_bounds, easu_clamp) on the same values — every pixel is the
// value the RGBA kernel of the element type stores.  The two ends that touch memory are this file's (include/fsr1_device_rgb.hpp):
//   staging  the planar kernel's texel-per-lane form with the texels three elements apart: one wave per footprint row, the row base
//            scalar, three element loads at stride 3 per texel, all of a wave's loads issued before the first conversion, edge
//            texels clamped per texel.  (The alternative for the fixed 35 x 11 footprint, a flat run of aligned dwords
//            de-interleaved into the records, was counted and not built: DESIGN.md section 3.5b.)
//   stores   exact 2x, WIDE: a wave's tile rows go through an LDS row buffer and leave as a flat run of aligned four-element stores
//            with an element-wise head and tail (rgb_store_run_rows).  Quads on the image border are filtered like all others and
//            only their stores are predicated.  WIDE = false — base, pitch or frame stride not a multiple of four elements, e.g. a
//            tightly packed odd width — stores the two pixels of a quad row element by element;
//            other ratios: a lane owns a column (easu_lane_column), three element stores per pixel.
#include "fsr1_device.h"
#include "fsr1_device_rgb.hpp"

namespace fsr1 {

size_t easu_lds_bytes(int fmt, int fp_w, int fp_h);

// bytes of the four waves' run buffers (exact 2x, WIDE)
template <int FMT>
constexpr size_t easu_rgb_run_bytes() { return (size_t)(kThreads / 64) * 2 * kRgbRunPitch * sizeof(typename Rgb3<FMT>::E); }

template <int FMT, bool EXACT, bool S2, bool HDR, bool WIDE>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(7, 8))) easu_rgb_kernel(const EasuArgs a) {
  typedef typename Rgb3<FMT>::E elem_t;
  constexpr int kPlanar = Rgb3Planar<FMT>::value;  // the element type's name for the shared staging
  constexpr int kS2W = kTileW / 2 + 3, kS2H = kTileH / 2 + 3;  // footprint of every exact-2x tile
  constexpr long long kPixel = 3 * sizeof(elem_t);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  EasuLds l = easu_lds_carve(smem, S2 ? kS2W * kS2H : a.fp_w * a.fp_h);

  const int tiles_per_frame = a.tiles_x * a.tiles_y;
  const int t = xcd_swizzle(blockIdx.x, tiles_per_frame * a.frames, a.xcd_shift);
  const int frame = t / tiles_per_frame;
  const int tf = t - frame * tiles_per_frame;
  const int ty = tf / a.tiles_x, tx = tf - ty * a.tiles_x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const char* const in_frame = a.in.base + (long long)frame * a.in.frame_stride;
  char* const out_frame = a.out.base + (long long)frame * a.out.frame_stride;
  const int W = a.out.width, H = a.out.height;
  const bool stream = (a.flags & FSR1_FLAG_OUTPUT_STREAMING) != 0;
  constexpr bool hdr = HDR;

  if constexpr (S2) {
    // tile (tx, ty) = output pixels [64 tx - 1, 64 tx + 62] x [16 ty - 1, 16 ty + 14] = 32 x 8 quads, quad (qx, qy) around texel
    // (32 tx - 1 + qx, 8 ty - 1 + qy): fsr1_easu_kernel.h
    const int ox0 = tx * kTileW - 1, oy0 = ty * kTileH - 1;
    l.fw = kS2W;
    easu_stage_footprint_planar<kPlanar, EXACT, kS2W, kS2H, 256, 3>(l, a.in, in_frame, tx * (kTileW / 2) - 2, ty * (kTileH / 2) - 2, kS2W, kS2H, tid);
    const int qx = lane & 31, qy = 2 * wave + (lane >> 5);
    const int oxa = ox0 + 2 * qx, oya = oy0 + 2 * qy;  // odd: the quad is {oxa, oxa + 1} x {oya, oya + 1}
    const bool xin0 = oxa >= 0 && oxa < W, xin1 = oxa + 1 < W, yin0 = oya >= 0 && oya < H, yin1 = oya + 1 < H;
    if (!__ballot((xin0 || xin1) && (yin0 || yin1))) return;  // (wave-uniform: the lanes of a wave leave together or not at all)
    const int f_idx = (qy + 1) * kS2W + (qx + 1);
    const float4_t A[4] = {l.ana[f_idx], l.ana[f_idx + 1], l.ana[f_idx + kS2W], l.ana[f_idx + kS2W + 1]};
    elem_t* const run = reinterpret_cast<elem_t*>(smem + easu_lds_region_bytes(kS2W * kS2H)) + wave * 2 * kRgbRunPitch;  // (WIDE)
    // row k (0 / 1) of the quad: for the wave, tile rows 4 wave + k and 4 wave + 2 + k
    auto store_row = [&](int k, rgbf_t left, rgbf_t right, bool row_in) {
      if constexpr (WIDE) {
        rgb_store_run_rows<FMT>(run, lane, left, right, out_frame, a.out.pitch, ox0, oy0 + 4 * wave + k, W, H, stream);
      } else {
        char* const o = out_frame + (long long)(oya + k) * a.out.pitch + (long long)oxa * kPixel;
        if (row_in && xin0) rgb_store1<FMT>(o, left, stream);
        if (row_in && xin1) rgb_store1<FMT>(o + kPixel, right, stream);
      }
    };
    EasuBounds m;
    if constexpr (!EXACT) {
      // the default arithmetic's row pairs (easu_quad_row): bounds of the first row's tap values
      rgbf_t q0, q1;
      easu_quad_row<true>(l, f_idx, 0.25f, A, m, q0, q1);
      store_row(0, easu_clamp<EXACT>(m, q0, hdr), easu_clamp<EXACT>(m, q1, hdr), yin0);
      easu_quad_row<false>(l, f_idx, 0.75f, A, m, q0, q1);
      store_row(1, easu_clamp<EXACT>(m, q0, hdr), easu_clamp<EXACT>(m, q1, hdr), yin1);
    } else {
      // EXACT: pixel by pixel with the quad's analyses shared and the bounds of the first pixel's taps
      const rgbf_t q00 = easu_quad_pixel<EXACT, true>(l, f_idx, 0.25f, 0.25f, A, m);
      const rgbf_t p00 = easu_clamp<EXACT>(m, q00, hdr);
      const rgbf_t p10 = easu_clamp<EXACT>(m, easu_quad_pixel<EXACT, false>(l, f_idx, 0.75f, 0.25f, A, m), hdr);
      store_row(0, p00, p10, yin0);
      const rgbf_t p01 = easu_clamp<EXACT>(m, easu_quad_pixel<EXACT, false>(l, f_idx, 0.25f, 0.75f, A, m), hdr);
      const rgbf_t p11 = easu_clamp<EXACT>(m, easu_quad_pixel<EXACT, false>(l, f_idx, 0.75f, 0.75f, A, m), hdr);
      store_row(1, p01, p11, yin1);
    }
    return;
  }

  // ---- any other ratio: fsr1_easu_kernel.h's generic form on the dense LDS layout ----
  constexpr int kRowsPerWave = kTileH / 4;
  const int ox0 = tx * kTileW, oy0 = ty * kTileH;
  const float c0x = as_f32(a.con[0]), c0y = as_f32(a.con[1]), c0z = as_f32(a.con[2]), c0w = as_f32(a.con[3]);
  const int oxl = min(ox0 + kTileW, W) - 1, oyl = min(oy0 + kTileH, H) - 1;
  const int fx0 = (int)floorf((float)ox0 * c0x + c0z) - 1;
  const int fy0 = (int)floorf((float)oy0 * c0y + c0w) - 1;
  const int fw = min((int)floorf((float)oxl * c0x + c0z) + 2 - fx0 + 1, a.fp_w);
  const int fh = min((int)floorf((float)oyl * c0y + c0w) + 2 - fy0 + 1, a.fp_h);
  l.fw = fw;
  easu_stage_footprint_planar<kPlanar, EXACT, 0, 0, 256, 3>(l, a.in, in_frame, fx0, fy0, fw, fh, tid);

  const int ox = ox0 + easu_lane_column(lane);
  if (ox >= W) return;
  char* const out_col = out_frame + (long long)ox * kPixel;
  float ppx = (float)ox * c0x + c0z;  // :324-326 (x part, shared by this lane's rows)
  const float fpx = floorf(ppx);
  ppx -= fpx;
  const int lx = (int)fpx - fx0;
#pragma unroll 1
  for (int r = 0; r < kRowsPerWave; ++r) {
    const int oy = oy0 + wave * kRowsPerWave + r;
    if (oy >= H) break;
    float ppy = (float)oy * c0y + c0w;
    const float fpy = floorf(ppy);
    ppy -= fpy;
    const EasuRowTerms yt = easu_row_terms(ppy);
    const int f_idx = ((int)fpy - fy0) * fw + lx;
    EasuBounds m;
    const rgbf_t p = easu_pixel_with_bounds<EXACT>(l, f_idx, ppx, yt, m);
    rgb_store1<FMT>(out_col + (long long)oy * a.out.pitch, easu_clamp<EXACT>(m, p, hdr), stream);
  }
}

template <int FMT, bool EXACT, bool S2, bool HDR, bool WIDE>
static hipError_t easu_rgb_launch_one(const EasuArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kThreads);
  const size_t lds = easu_lds_bytes(FMT, a.fp_w, a.fp_h) + (S2 && WIDE ? easu_rgb_run_bytes<FMT>() : 0);
  if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&easu_rgb_kernel<FMT, EXACT, S2, HDR, WIDE>), lds); e != hipSuccess) return e;
  hipLaunchKernelGGL((easu_rgb_kernel<FMT, EXACT, S2, HDR, WIDE>), grid, block, lds, stream, a);
  return hipGetLastError();
}

// s2: the exact-2x variant (the host has checked con0 and laid the grid out for the shifted tiles); wide: its run stores (the host
// has checked the output's base, pitch and frame stride against four elements).  The generic variant has no wide form.
hipError_t easu_rgb_launch(const EasuArgs& a, int fmt, bool exact, bool s2, bool wide, hipStream_t stream) {
  const bool hdr = (a.flags & FSR1_FLAG_HDR_SQUARE) != 0;
#define FSR1_RGB_H(F, E, S, V) return hdr ? easu_rgb_launch_one<F, E, S, true, V>(a, stream) : easu_rgb_launch_one<F, E, S, false, V>(a, stream)
#define FSR1_RGB_E(F)                               \
  do {                                              \
    if (s2 && wide) {                               \
      if (exact) FSR1_RGB_H(F, true, true, true);   \
      FSR1_RGB_H(F, false, true, true);             \
    }                                               \
    if (s2) {                                       \
      if (exact) FSR1_RGB_H(F, true, true, false);  \
      FSR1_RGB_H(F, false, true, false);            \
    }                                               \
    if (exact) FSR1_RGB_H(F, true, false, false);   \
    FSR1_RGB_H(F, false, false, false);             \
  } while (0)
  switch (fmt) {
    case FSR1_FORMAT_RGB16F: FSR1_RGB_E(FSR1_FORMAT_RGB16F);
    case FSR1_FORMAT_RGB32F: FSR1_RGB_E(FSR1_FORMAT_RGB32F);
    case FSR1_FORMAT_RGB8_UNORM: FSR1_RGB_E(FSR1_FORMAT_RGB8_UNORM);
    default: return hipErrorInvalidValue;
  }
#undef FSR1_RGB_E
#undef FSR1_RGB_H
}

}  // namespace fsr1
