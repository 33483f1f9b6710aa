// EASU on a decoder's NV12 frame (FSR1_FORMAT_NV12: an 8-bit Y plane and a half-resolution plane of Cb, Cr pairs) into planar RGB
// (FSR1_FORMAT_RGB16F_PLANAR / RGB32F_PLANAR / RGB8_UNORM_PLANAR): chroma reconstruction and the YCbCr -> RGB conversion pinned in
// fsr1_hip.h happen while the footprint is staged, once per INPUT texel, so the frame never exists as RGB in memory.
//
// The filter is fsr1_easu_planar.hip's: the same 64 x 16 tiles of four waves in the XCD-aware order, the same LDS records, the same
// per-pixel functions, the same plane stores (planar_store_quad_row / planar_store_quad_row_u8 / planar_store1) — the image it
// stores is the one the planar kernel of the output's format stores for the converted frame, bit for bit.  What is this file's is
// phase 1 (include/fsr1_device_nv12.hpp): the tile's chroma pairs go through a small LDS region of their own behind the records
// (320 bytes at exactly 2x), each lane loads one Y byte per texel, and the output format is free of the input's.
//
// FSR1_FORMAT_P010 / P016 (the same arrangement in 16-bit words) are the same kernel with WORD = uint16_t: 32-bit pairs in LDS (640
// bytes at exactly 2x), one Y word per texel, the depth a run-time shift — 36 more instantiations for both depths together.
#include "fsr1_device.h"
#include "fsr1_device_nv12.hpp"

namespace fsr1 {

// pair_bytes: 2 (NV12) or 4 (P010 / P016)
size_t easu_nv12_lds_bytes(int fp_w, int fp_h, int pair_bytes) { return easu_lds_region_bytes((size_t)fp_w * fp_h) + nv12_chroma_lds_bytes(fp_w, fp_h, pair_bytes); }

template <int FOUT, bool EXACT, bool S2, bool HDR, bool WIDE, class WORD>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(7, 8))) easu_nv12_kernel(const EasuArgs a, const Nv12View yc) {
  typedef typename Plane<FOUT>::E elem_t;
  constexpr int kS2W = kTileW / 2 + 3, kS2H = kTileH / 2 + 3;  // footprint of every exact-2x tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int capacity = S2 ? kS2W * kS2H : a.fp_w * a.fp_h;
  EasuLds l = easu_lds_carve(smem, capacity);
  typedef typename Nv12Pair<WORD>::T pair_t;
  pair_t* const pairs = reinterpret_cast<pair_t*>(smem + easu_lds_region_bytes((size_t)capacity));

  const int tiles_per_frame = a.tiles_x * a.tiles_y;
  const int t = xcd_swizzle(blockIdx.x, tiles_per_frame * a.frames, a.xcd_shift);
  const int frame = t / tiles_per_frame;
  const int tf = t - frame * tiles_per_frame;
  const int ty = tf / a.tiles_x, tx = tf - ty * a.tiles_x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const char* const in_frame = a.in.base + (long long)frame * a.in.frame_stride;
  char* const out_frame = a.out.base + (long long)frame * a.out.frame_stride;
  const long long ops = plane_stride(a.out);
  const int W = a.out.width, H = a.out.height;
  const bool stream = (a.flags & FSR1_FLAG_OUTPUT_STREAMING) != 0;
  constexpr bool hdr = HDR;

  if constexpr (S2) {
    // the shifted tiles and 2 x 2 quads of the exact-2x variant: fsr1_easu_planar.hip, fsr1_easu_kernel.h
    const int ox0 = tx * kTileW - 1, oy0 = ty * kTileH - 1;
    l.fw = kS2W;
    easu_stage_footprint_nv12<EXACT, kS2W, kS2H, kThreads, WORD>(l, pairs, a.in, yc, in_frame, tx * (kTileW / 2) - 2, ty * (kTileH / 2) - 2, kS2W, kS2H, tid);
    const int qx = lane & 31, qy = 2 * wave + (lane >> 5);
    const int oxa = ox0 + 2 * qx, oya = oy0 + 2 * qy;
    const bool xin0 = oxa >= 0 && oxa < W, xin1 = oxa + 1 < W, xin2 = oxa + 2 < W, yin0 = oya >= 0 && oya < H, yin1 = oya + 1 < H;
    if (!__ballot((xin0 || xin1) && (yin0 || yin1))) return;  // (wave-uniform)
    const int f_idx = (qy + 1) * kS2W + (qx + 1);
    char* const o0 = out_frame + (long long)oya * a.out.pitch + (long long)oxa * (long long)sizeof(elem_t);
    const float4_t A[4] = {l.ana[f_idx], l.ana[f_idx + 1], l.ana[f_idx + kS2W], l.ana[f_idx + kS2W + 1]};
    auto store_row = [&](char* o, rgbf_t left, rgbf_t right, bool row_in) {
      if constexpr (FOUT == FSR1_FORMAT_RGB8_UNORM_PLANAR) planar_store_quad_row_u8<WIDE>(o, ops, left, right, qx, oxa, W, row_in, stream);
      else planar_store_quad_row<FOUT, WIDE>(o, ops, left, right, qx, row_in, xin0, xin1, xin2, stream);
    };
    EasuBounds m;
    if constexpr (!EXACT) {
      rgbf_t q0, q1;
      easu_quad_row<true>(l, f_idx, 0.25f, A, m, q0, q1);
      store_row(o0, easu_clamp<EXACT>(m, q0, hdr), easu_clamp<EXACT>(m, q1, hdr), yin0);
      easu_quad_row<false>(l, f_idx, 0.75f, A, m, q0, q1);
      store_row(o0 + a.out.pitch, easu_clamp<EXACT>(m, q0, hdr), easu_clamp<EXACT>(m, q1, hdr), yin1);
    } else {
      const rgbf_t q00 = easu_quad_pixel<EXACT, true>(l, f_idx, 0.25f, 0.25f, A, m);
      const rgbf_t p00 = easu_clamp<EXACT>(m, q00, hdr);
      const rgbf_t p10 = easu_clamp<EXACT>(m, easu_quad_pixel<EXACT, false>(l, f_idx, 0.75f, 0.25f, A, m), hdr);
      store_row(o0, p00, p10, yin0);
      const rgbf_t p01 = easu_clamp<EXACT>(m, easu_quad_pixel<EXACT, false>(l, f_idx, 0.25f, 0.75f, A, m), hdr);
      const rgbf_t p11 = easu_clamp<EXACT>(m, easu_quad_pixel<EXACT, false>(l, f_idx, 0.75f, 0.75f, A, m), hdr);
      store_row(o0 + a.out.pitch, p01, p11, yin1);
    }
    return;
  }

  // ---- any other ratio: the generic form on the dense LDS layout, a lane per output column ----
  constexpr int kRowsPerWave = kTileH / 4;
  const int ox0 = tx * kTileW, oy0 = ty * kTileH;
  const float c0x = as_f32(a.con[0]), c0y = as_f32(a.con[1]), c0z = as_f32(a.con[2]), c0w = as_f32(a.con[3]);
  const int oxl = min(ox0 + kTileW, W) - 1, oyl = min(oy0 + kTileH, H) - 1;
  const int fx0 = (int)floorf((float)ox0 * c0x + c0z) - 1;
  const int fy0 = (int)floorf((float)oy0 * c0y + c0w) - 1;
  const int fw = min((int)floorf((float)oxl * c0x + c0z) + 2 - fx0 + 1, a.fp_w);
  const int fh = min((int)floorf((float)oyl * c0y + c0w) + 2 - fy0 + 1, a.fp_h);
  l.fw = fw;
  easu_stage_footprint_nv12<EXACT, 0, 0, kThreads, WORD>(l, pairs, a.in, yc, in_frame, fx0, fy0, fw, fh, tid);

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
    const EasuRowTerms yt = easu_row_terms(ppy);
    const int f_idx = ((int)fpy - fy0) * fw + lx;
    EasuBounds m;
    const rgbf_t p = easu_pixel_with_bounds<EXACT>(l, f_idx, ppx, yt, m);
    planar_store1<FOUT>(out_col + (long long)oy * a.out.pitch, ops, easu_clamp<EXACT>(m, p, hdr), stream);
  }
}

template <int FOUT, bool EXACT, bool S2, bool HDR, bool WIDE, class WORD>
static hipError_t easu_nv12_launch_word(const EasuArgs& a, const Nv12View& yc, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kThreads);
  const size_t lds = easu_nv12_lds_bytes(a.fp_w, a.fp_h, (int)sizeof(typename Nv12Pair<WORD>::T));
  if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&easu_nv12_kernel<FOUT, EXACT, S2, HDR, WIDE, WORD>), lds); e != hipSuccess) return e;
  hipLaunchKernelGGL((easu_nv12_kernel<FOUT, EXACT, S2, HDR, WIDE, WORD>), grid, block, lds, stream, a, yc);
  return hipGetLastError();
}

// the word width by the input's format: yc.shift < 0 marks NV12's bytes
template <int FOUT, bool EXACT, bool S2, bool HDR, bool WIDE>
static hipError_t easu_nv12_launch_one(const EasuArgs& a, const Nv12View& yc, hipStream_t stream) {
  if (yc.shift < 0) return easu_nv12_launch_word<FOUT, EXACT, S2, HDR, WIDE, uint8_t>(a, yc, stream);
  return easu_nv12_launch_word<FOUT, EXACT, S2, HDR, WIDE, uint16_t>(a, yc, stream);
}

// fout: the planar format of the output; s2 / wide as for easu_planar_launch (the host has checked the OUTPUT's base, pitch, plane
// and frame stride against the wide stores; the input is read one and two bytes at a time whatever its alignment).
// chroma_offset: bytes from a frame's Y plane to its CbCr plane, resolved and checked by the host.
// bits: 8 = NV12's bytes; 10 / 16 = P010 / P016's words (the host has checked base, pitch, chroma offset and frame stride against the
// aligned dword a pair then is).
hipError_t easu_nv12_launch(const EasuArgs& a, const fsr1_ycbcr& ycbcr, long long chroma_offset, int bits, int fout, bool exact, bool s2, bool wide, hipStream_t stream) {
  Nv12View yc;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) yc.m[r][c] = ycbcr.m[r][c];
    yc.bias[r] = ycbcr.bias[r];
  }
  yc.siting = ycbcr.siting;
  yc.chroma_offset = chroma_offset;
  yc.shift = bits == 8 ? -1 : 16 - bits;
  const bool hdr = (a.flags & FSR1_FLAG_HDR_SQUARE) != 0;
#define FSR1_NV12_H(F, E, S, V) return hdr ? easu_nv12_launch_one<F, E, S, true, V>(a, yc, stream) : easu_nv12_launch_one<F, E, S, false, V>(a, yc, stream)
#define FSR1_NV12_E(F)                               \
  do {                                               \
    if (s2 && wide) {                                \
      if (exact) FSR1_NV12_H(F, true, true, true);   \
      FSR1_NV12_H(F, false, true, true);             \
    }                                                \
    if (s2) {                                        \
      if (exact) FSR1_NV12_H(F, true, true, false);  \
      FSR1_NV12_H(F, false, true, false);            \
    }                                                \
    if (exact) FSR1_NV12_H(F, true, false, false);   \
    FSR1_NV12_H(F, false, false, false);             \
  } while (0)
  switch (fout) {
    case FSR1_FORMAT_RGB16F_PLANAR: FSR1_NV12_E(FSR1_FORMAT_RGB16F_PLANAR);
    case FSR1_FORMAT_RGB32F_PLANAR: FSR1_NV12_E(FSR1_FORMAT_RGB32F_PLANAR);
    case FSR1_FORMAT_RGB8_UNORM_PLANAR: FSR1_NV12_E(FSR1_FORMAT_RGB8_UNORM_PLANAR);
    default: return hipErrorInvalidValue;
  }
#undef FSR1_NV12_E
#undef FSR1_NV12_H
}

}  // namespace fsr1
