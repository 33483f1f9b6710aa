// EASU on single-channel images (FSR1_FORMAT_R16F / R32F / R8_UNORM): the Y plane of a decoded frame, a (N,1,H,W) tensor, greyscale
// imagery — one channel in, one out, no replication into RGBA.
//
// Every stored value is channel R of what fsr1_easu.hip stores for the image (L, L, L, 1), default arithmetic included; the kernel
// around that arithmetic is its own (include/fsr1_device_mono.hpp):
//   tiles    64 x 16 output pixels, four waves, the XCD-aware tile order.  At exactly 2x a lane owns a 2 x 2 quad of the shifted tile
//            (pixels 64 tx - 1 .. 64 tx + 62, fsr1_easu_kernel.h) and the footprint is a compile-time 35 x 11 texels; at any other
//            ratio a lane owns a column (easu_lane_column) and a wave four rows.
//   LDS      a value plane of one binary32 per texel + the 16-byte analysis records: 20 B per texel against the RGBA kernels' 32 —
//            7.7 KB for the exact-2x footprint, so LDS would admit 20 workgroups per CU; what limits residency is the SIMD's wave
//            slots: 8 workgroups of four waves per CU = 8 waves per SIMD, which the kernels' <= 64 VGPRs allow.
//   staging  one wave per footprint row, one element load per texel, all of a wave's loads issued before the first conversion; the
//            analyses from lumas computed by the reference's expression B*0.5 + (R*0.5 + G) of (L, L, L) — not 2 L.
//   filter   exact 2x: the quad's 12-tap window is read from LDS ONCE, into twelve registers (six ds_read2_b32), and serves its four
//            pixels, as do the four analyses and the dering bounds — 28 dwords of LDS reads per quad where the RGBA row-pair form reads
//            112; one accumulator and the weight sum per pixel.  Other ratios: the window per pixel, the bounds of its values.
//   stores   exact 2x: the lane exchange to even-aligned pairs (binary16 4 B, binary32 8 B; 8-bit: dwords of four columns from the even
//            quad columns) when base, pitch and stride allow (WIDE), element by element otherwise; border quads are filtered like all
//            others (their window lies in the clamped footprint) and only their stores are predicated.  Other ratios: one element per
//            lane and row, 64 contiguous elements per wave (a pair form for them: not built, unmeasured).
#include "fsr1_device.h"
#include "fsr1_device_mono.hpp"

namespace fsr1 {

size_t easu_mono_lds_bytes(int fp_w, int fp_h) { return easu_mono_lds_region_bytes((size_t)fp_w * fp_h); }

// amdgpu_waves_per_eu: eight waves per SIMD (<= 64 VGPRs) — except the EXACT exact-2x variant, whose reference-order filter beside the
// quad's window and four full analysis records needs 66 - 70: seven waves there (at 64 it spills two to four registers).
template <int FMT, bool EXACT, bool S2, bool HDR, bool WIDE>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(EXACT && S2 ? 7 : 8, 8))) easu_mono_kernel(const EasuArgs a) {
  typedef typename Mono<FMT>::U elem_t;
  constexpr int kS2W = kTileW / 2 + 3, kS2H = kTileH / 2 + 3;  // footprint of every exact-2x tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  EasuMonoLds l = easu_mono_lds_carve(smem, S2 ? kS2W * kS2H : a.fp_w * a.fp_h);

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
    easu_stage_footprint_mono<FMT, EXACT, kS2W, kS2H>(l, a.in, in_frame, tx * (kTileW / 2) - 2, ty * (kTileH / 2) - 2, kS2W, kS2H, tid);
    const int qx = lane & 31, qy = 2 * wave + (lane >> 5);
    const int oxa = ox0 + 2 * qx, oya = oy0 + 2 * qy;  // odd: the quad is {oxa, oxa + 1} x {oya, oya + 1}
    const bool xin = (oxa >= 0 && oxa < W) || oxa + 1 < W, yin0 = oya >= 0 && oya < H, yin1 = oya + 1 < H;
    if (!__ballot(xin && (yin0 || yin1))) return;  // (wave-uniform: the lanes of a wave leave together or not at all)
    const int f_idx = (qy + 1) * kS2W + (qx + 1);
    char* const o0 = out_frame + (long long)oya * a.out.pitch + (long long)oxa * (long long)sizeof(elem_t);
    const EasuMonoWindow w = easu_mono_window(l, f_idx);
    const float4_t A[4] = {l.ana[f_idx], l.ana[f_idx + 1], l.ana[f_idx + kS2W], l.ana[f_idx + kS2W + 1]};
    const EasuMonoBounds m = easu_mono_bounds(w);
    auto ana = [&](int k) { return A[k]; };
    auto row = [&](char* o, float ppy, bool row_in) {
      const EasuRowTerms yt = easu_row_terms(ppy);
      const float left = easu_mono_clamp<EXACT>(m, easu_mono_filter<EXACT>(w, ana, 0.25f, yt), hdr);
      const float right = easu_mono_clamp<EXACT>(m, easu_mono_filter<EXACT>(w, ana, 0.75f, yt), hdr);
      mono_store_quad_row<FMT, WIDE>(o, left, right, qx, oxa, W, row_in, stream);
    };
    row(o0, 0.25f, yin0);
    row(o0 + a.out.pitch, 0.75f, yin1);
    return;
  }

  // ---- any other ratio: a lane owns a column, a wave four rows of the tile ----
  constexpr int kRowsPerWave = kTileH / 4;
  const int ox0 = tx * kTileW, oy0 = ty * kTileH;
  const float c0x = as_f32(a.con[0]), c0y = as_f32(a.con[1]), c0z = as_f32(a.con[2]), c0w = as_f32(a.con[3]);
  const int oxl = min(ox0 + kTileW, W) - 1, oyl = min(oy0 + kTileH, H) - 1;
  const int fx0 = (int)floorf((float)ox0 * c0x + c0z) - 1;
  const int fy0 = (int)floorf((float)oy0 * c0y + c0w) - 1;
  const int fw = min((int)floorf((float)oxl * c0x + c0z) + 2 - fx0 + 1, a.fp_w);
  const int fh = min((int)floorf((float)oyl * c0y + c0w) + 2 - fy0 + 1, a.fp_h);
  l.fw = fw;
  easu_stage_footprint_mono<FMT, EXACT>(l, a.in, in_frame, fx0, fy0, fw, fh, tid);

  const int ox = ox0 + easu_lane_column(lane);
  if (ox >= W) return;
  char* const out_col = out_frame + (size_t)ox * sizeof(elem_t);
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
    const float p = easu_mono_pixel<EXACT>(l, ((int)fpy - fy0) * fw + lx, ppx, easu_row_terms(ppy), hdr);
    store_out<sizeof(elem_t)>(out_col + (long long)oy * a.out.pitch, Mono<FMT>::store(p), stream);
  }
}

template <int FMT, bool EXACT, bool S2, bool HDR, bool WIDE>
static hipError_t easu_mono_launch_one(const EasuArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kThreads);
  const size_t lds = easu_mono_lds_bytes(a.fp_w, a.fp_h);
  if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&easu_mono_kernel<FMT, EXACT, S2, HDR, WIDE>), lds); e != hipSuccess) return e;
  hipLaunchKernelGGL((easu_mono_kernel<FMT, EXACT, S2, HDR, WIDE>), grid, block, lds, stream, a);
  return hipGetLastError();
}

// s2: the exact-2x variant (the host has checked con0 and laid the grid out for the shifted tiles); wide: its pair stores (the host has
// checked the output's base, pitch and frame stride against two elements; 8-bit: its dword stores, against four).  The generic variant
// has no wide form.
hipError_t easu_mono_launch(const EasuArgs& a, int fmt, bool exact, bool s2, bool wide, hipStream_t stream) {
  const bool hdr = (a.flags & FSR1_FLAG_HDR_SQUARE) != 0;
#define FSR1_MONO_H(F, E, S, V) return hdr ? easu_mono_launch_one<F, E, S, true, V>(a, stream) : easu_mono_launch_one<F, E, S, false, V>(a, stream)
#define FSR1_MONO_E(F)                               \
  do {                                               \
    if (s2 && wide) {                                \
      if (exact) FSR1_MONO_H(F, true, true, true);   \
      FSR1_MONO_H(F, false, true, true);             \
    }                                                \
    if (s2) {                                        \
      if (exact) FSR1_MONO_H(F, true, true, false);  \
      FSR1_MONO_H(F, false, true, false);            \
    }                                                \
    if (exact) FSR1_MONO_H(F, true, false, false);   \
    FSR1_MONO_H(F, false, false, false);             \
  } while (0)
  switch (fmt) {
    case FSR1_FORMAT_R16F: FSR1_MONO_E(FSR1_FORMAT_R16F);
    case FSR1_FORMAT_R32F: FSR1_MONO_E(FSR1_FORMAT_R32F);
    case FSR1_FORMAT_R8_UNORM: FSR1_MONO_E(FSR1_FORMAT_R8_UNORM);
    default: return hipErrorInvalidValue;
  }
#undef FSR1_MONO_E
#undef FSR1_MONO_H
}

}  // namespace fsr1
