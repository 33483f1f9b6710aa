// RCAS on planar RGB input (FSR1_FORMAT_RGB16F_PLANAR / RGB32F_PLANAR / RGB8_UNORM_PLANAR) straight into an NV12 surface: the
// RGB -> YCbCr conversion and the 4:2:0 decimation pinned in fsr1_hip.h happen in the store, and the sharpened image never exists as
// RGB in memory.  RCAS is the pass bound by its bytes: this store is 1.5 B per pixel where uint8 planes store
// 3 and fp16 planes 6, and the conversion is about two dozen VALU operations per pixel in a kernel that has them to spare.
//
// The strip walk is fsr1_rcas_planar_kernel.h's (256-column waves, four columns per lane, DPP taps, register ring, strips walking
// down and up alternately); what is this file's own is what becomes of a finished row:
//   * a lane's four columns start on a multiple of four — two whole chroma pairs, no cross-lane traffic; strip origins and heights are
//     multiples of 8 — whole row pairs, no cross-strip state;
//   * Y: four conversions, merged into ONE dword store per lane and row;
//   * chroma: the first row of a pair the walk reaches (the even one walking down, the odd one walking up) leaves its two horizontal
//     sums per channel in six registers; the second adds its own (s0 + s1 is commutative: both directions give the same bits), scales,
//     converts to two (Cb, Cr) pairs and issues ONE dword store per lane per TWO rows;
//   * the siting is a run-time, wave-uniform choice between the box sample and the even row's even pixel (six v_cndmask per two rows):
//     no instantiation of its own, the kernel count is the planar kernel's (3 inputs x EXACT x OPTS x WIDE x the rings = 40);
//   * in the predicated body an odd last row flushes with itself as its partner and an odd last column pairs with itself (the clamp of
//     the pinned definition); ragged lanes, and every lane where WIDE is false, store bytes and 16-bit pairs: no byte outside the
//     w x h luma bytes and the 2 cw x ch pair bytes of a frame is written, and no access is wider than its alignment.
// FSR1_FORMAT_P010 / P016 (16-bit words, the code in the upper bits) are a second sink on the same walk, WORD = uint16_t: the row-pair
// logic above is shared word for word, the depth is two kernel arguments (the maximum code and the shift), and what differs is the width
// of what a lane stores — its four Y words are 8 bytes, its two pairs are 8 bytes: ONE 8-byte store per lane and row, ONE per lane per
// two rows where the host found base, pitch, chroma offset and frame stride multiples of 8 (a lane's columns start on a multiple of
// four: 8 bytes); otherwise 16-bit Y stores and one aligned dword per pair (the format's contract: multiples of 4 everywhere).
#include <string.h>

#include "fsr1_device_nv12_out.hpp"
#include "fsr1_rcas_planar_kernel.h"

namespace fsr1 {

struct RcasNv12Args : RcasArgs {  // `out`: the view of the Y plane, whose pitch and frame stride the chroma plane shares
  Rgb2YcbcrView yc;
};

template <bool WIDE, class WORD>
struct RcasNv12Store {
  typedef uint32_t dword2_t __attribute__((ext_vector_type(2)));
  static constexpr bool kWords = sizeof(WORD) == 2;
  const RcasNv12Args& a;
  char* const out_frame;
  const bool stream, replicate;
  rgb_t held[2];  // of the pair's first row, per chroma pair of the lane: its horizontal sums, or its even pixel (REPLICATE, walking down)
  __device__ __forceinline__ RcasNv12Store(const RcasNv12Args& args, int frame)
      : a(args), out_frame(args.out.base + (long long)frame * args.out.frame_stride),
        stream((args.flags & FSR1_FLAG_OUTPUT_STREAMING) != 0), replicate(args.yc.siting == FSR1_CHROMA_REPLICATE) {}

  __device__ __forceinline__ rgb_t pick(rgb_t even_pixel, rgb_t box) const {
    return rgb_t{replicate ? even_pixel.r : box.r, replicate ? even_pixel.g : box.g, replicate ? even_pixel.b : box.b};
  }
  // the chroma row of image rows y & ~1, y | 1 from the lane's two samples
  __device__ __forceinline__ void pairs(int y, int col, const bool (&ok)[4], rgb_t a0, rgb_t a1) const {
    char* const dst = out_frame + a.yc.chroma_offset + (long long)(y >> 1) * a.out.pitch + rcas_planar_zext((uint32_t)col * (uint32_t)sizeof(WORD));
    if constexpr (kWords) {
      const uint32_t p0 = p016_pair_words(a.yc, a0), p1 = p016_pair_words(a.yc, a1);
      if (WIDE && ok[2]) {  // (both pairs exist: their eight bytes lie within the 4 cw of the row)
        store_out<8>(dst, dword2_t{p0, p1}, stream);
      } else {
        if (ok[0]) store_out<4>(dst, p0, stream);
        if (ok[2]) store_out<4>(dst + 4, p1, stream);
      }
      return;
    }
    const uint32_t p0 = nv12_pair_code(a.yc, a0), p1 = nv12_pair_code(a.yc, a1);
    if (WIDE && ok[2]) {  // (column col + 2 inside: both pairs exist, and their four bytes lie within the 2 cw of the row)
      store_out<4>(dst, p0 | (p1 << 16), stream);
    } else {
      if (ok[0]) store_out<2>(dst, (uint16_t)p0, stream);
      if (ok[2]) store_out<2>(dst + 2, (uint16_t)p1, stream);
    }
  }
  template <bool INTERIOR, bool UP>
  __device__ __forceinline__ void row(int k, int y, int col, uint32_t, const bool (&ok)[4], rgb_t o0, rgb_t o1, rgb_t o2, rgb_t o3) {
    if constexpr (kWords) {
      char* const dst = out_frame + (long long)y * a.out.pitch + rcas_planar_zext((uint32_t)col * 2u);
      const uint32_t c0 = p016_luma_word(a.yc, o0), c1 = p016_luma_word(a.yc, o1), c2 = p016_luma_word(a.yc, o2), c3 = p016_luma_word(a.yc, o3);
      if (WIDE && ok[3]) {
        store_out<8>(dst, dword2_t{c0 | (c1 << 16), c2 | (c3 << 16)}, stream);
      } else {
        if (ok[0]) store_out<2>(dst, (uint16_t)c0, stream);
        if (ok[1]) store_out<2>(dst + 2, (uint16_t)c1, stream);
        if (ok[2]) store_out<2>(dst + 4, (uint16_t)c2, stream);
        if (ok[3]) store_out<2>(dst + 6, (uint16_t)c3, stream);
      }
    } else {
      char* const dst = out_frame + (long long)y * a.out.pitch + rcas_planar_zext((uint32_t)col);
      const uint32_t c0 = nv12_luma_code(a.yc, o0), c1 = nv12_luma_code(a.yc, o1), c2 = nv12_luma_code(a.yc, o2), c3 = nv12_luma_code(a.yc, o3);
      if (WIDE && ok[3]) {
        store_out<4>(dst, c0 | (c1 << 8) | (c2 << 16) | (c3 << 24), stream);
      } else {
        if (ok[0]) store_out<1>(dst, (uint8_t)c0, stream);
        if (ok[1]) store_out<1>(dst + 1, (uint8_t)c1, stream);
        if (ok[2]) store_out<1>(dst + 2, (uint8_t)c2, stream);
        if (ok[3]) store_out<1>(dst + 3, (uint8_t)c3, stream);
      }
    }
    // an odd last column stands in for its missing neighbour (ok[] is true throughout an interior strip)
    const rgb_t s0 = nv12_sum(o0, ok[1] ? o1 : o0), s1 = nv12_sum(o2, ok[3] ? o3 : o2);
    if ((k & 1) == 0) {  // static: the first row of its pair — the even one unless the strip walks up
      if (!INTERIOR && y == a.in.height - 1) {  // an odd last row is its own partner
        pairs(y, col, ok, pick(o0, nv12_box(s0, s0)), pick(o2, nv12_box(s1, s1)));
      } else {
        held[0] = UP ? s0 : pick(o0, s0);
        held[1] = UP ? s1 : pick(o2, s1);
      }
    } else {  // the second: walking up it is the even row, whose even pixels REPLICATE takes
      pairs(y, col, ok, pick(UP ? o0 : held[0], nv12_box(held[0], s0)), pick(UP ? o2 : held[1], nv12_box(held[1], s1)));
    }
  }
};

// FIN: the planar format of the input.  OPTS = false: the plain pass (no denoise / HDR square), flags compiled out.
template <int FIN, bool EXACT, bool OPTS, bool WIDE, int RING, class WORD>
__global__ void __launch_bounds__(kRcasPlanarThreads) rcas_nv12_kernel(const RcasNv12Args a) {
  rcas_planar_workgroup<FIN, EXACT, OPTS, WIDE, RING, RcasNv12Store<WIDE, WORD>>(a);
}

template <int FIN, bool EXACT, bool OPTS, bool WIDE, class WORD>
static void rcas_nv12_launch_word(const RcasNv12Args& a, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kRcasPlanarThreads);
  if constexpr (FIN != FSR1_FORMAT_RGB8_UNORM_PLANAR) {
    if (rcas_planar_shallow_ring(a, FIN)) {
      hipLaunchKernelGGL((rcas_nv12_kernel<FIN, EXACT, OPTS, WIDE, 2, WORD>), grid, block, 0, stream, a);
      return;
    }
  }
  hipLaunchKernelGGL((rcas_nv12_kernel<FIN, EXACT, OPTS, WIDE, 4, WORD>), grid, block, 0, stream, a);
}

template <int FIN, bool EXACT, bool OPTS, bool WIDE>
static void rcas_nv12_launch_one(const RcasNv12Args& a, int bits, hipStream_t stream) {
  if (bits == 8) rcas_nv12_launch_word<FIN, EXACT, OPTS, WIDE, uint8_t>(a, stream);
  else rcas_nv12_launch_word<FIN, EXACT, OPTS, WIDE, uint16_t>(a, stream);
}

// r: the checked views (out = the Y plane) and the planar geometry; wide: the input's four-element accesses AND dword stores into both
// planes of the surface (the host has checked base, pitch, chroma offset and frame stride against them).
// bits: 8 = NV12's bytes; 10 / 16 = P010 / P016's words, whose wide stores are 8 bytes.
hipError_t rcas_nv12_launch(const RcasArgs& r, const fsr1_rgb2ycbcr& yc, long long chroma_offset, int bits, int fin, bool exact, bool wide, hipStream_t stream) {
  RcasNv12Args a;
  static_cast<RcasArgs&>(a) = r;
  memcpy(a.yc.m, yc.m, sizeof a.yc.m);
  memcpy(a.yc.bias, yc.bias, sizeof a.yc.bias);
  a.yc.siting = yc.siting;
  a.yc.chroma_offset = chroma_offset;
  a.yc.max_code = (float)((1u << bits) - 1u);
  a.yc.shift = bits == 8 ? 0u : (uint32_t)(16 - bits);
  const bool opts = (a.flags & (FSR1_FLAG_RCAS_DENOISE | FSR1_FLAG_HDR_SQUARE)) != 0;
#define FSR1_RCASN(F, E, O, V) rcas_nv12_launch_one<F, E, O, V>(a, bits, stream)
#define FSR1_RCASN_V(F, E, O) do { if (wide) FSR1_RCASN(F, E, O, true); else FSR1_RCASN(F, E, O, false); } while (0)
#define FSR1_RCASN_O(F, E) do { if (opts) FSR1_RCASN_V(F, E, true); else FSR1_RCASN_V(F, E, false); } while (0)
#define FSR1_RCASN_E(F) do { if (exact) FSR1_RCASN_O(F, true); else FSR1_RCASN_O(F, false); } while (0)
  switch (fin) {
    case FSR1_FORMAT_RGB16F_PLANAR: FSR1_RCASN_E(FSR1_FORMAT_RGB16F_PLANAR); break;
    case FSR1_FORMAT_RGB32F_PLANAR: FSR1_RCASN_E(FSR1_FORMAT_RGB32F_PLANAR); break;
    case FSR1_FORMAT_RGB8_UNORM_PLANAR: FSR1_RCASN_E(FSR1_FORMAT_RGB8_UNORM_PLANAR); break;
    default: return hipErrorInvalidValue;
  }
#undef FSR1_RCASN_E
#undef FSR1_RCASN_O
#undef FSR1_RCASN_V
#undef FSR1_RCASN
  return hipGetLastError();
}

}  // namespace fsr1
