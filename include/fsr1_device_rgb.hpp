// Packed 3-channel RGB storage (FSR1_FORMAT_RGB16F / RGB32F / RGB8_UNORM) for the tiled forms: R, G, B interleaved with no alpha,
// three elements per pixel, rows `pitch` bytes apart — a (N,H,W,3) tensor or a channels_last (N,3,H,W) one.  The filters are the
// ones of fsr1_device_easu.hpp / fsr1_device_rcas.hpp on the same LDS records and registers; what differs is the two ends that touch
// memory.  A pixel is three elements, so no power-of-two access holds a whole number of pixels — but FOUR pixels are exactly three
// accesses of four elements (4 / 8 / 16 bytes), aligned wherever the row is: this header holds that group of twelve elements and
// the flat run store of the exact-2x EASU tiles.
//
// Every global access is naturally aligned to its own width: a kernel takes a four-element access only where its instantiation
// (WIDE) was chosen by a host that has checked base, pitch and frame stride against that width.
#pragma once
#include "fsr1_device_planar.hpp"

namespace fsr1 {

// Elements, their conversions and the four-element access are the planar format's of the same element type (Plane<>: 8-bit codes
// under the conversions pinned for RGBA8_UNORM); P2 = two adjacent elements as one LDS access.
template <int FMT> struct Rgb3;  // FMT = a 3-channel fsr1_format
template <> struct Rgb3<FSR1_FORMAT_RGB16F> : Plane<FSR1_FORMAT_RGB16F_PLANAR> {
  typedef V2 P2;
  static __device__ __forceinline__ P2 make2(E a, E b) { return P2{a, b}; }
};
template <> struct Rgb3<FSR1_FORMAT_RGB32F> : Plane<FSR1_FORMAT_RGB32F_PLANAR> {
  typedef V2 P2;
  static __device__ __forceinline__ P2 make2(E a, E b) { return P2{a, b}; }
};
template <> struct Rgb3<FSR1_FORMAT_RGB8_UNORM> : Plane<FSR1_FORMAT_RGB8_UNORM_PLANAR> {
  typedef uint16_t P2;
  static __device__ __forceinline__ P2 make2(E a, E b) { return (P2)(a | (b << 8)); }
};
template <int FMT> struct Rgb3Planar { static constexpr int value = FMT - FSR1_FORMAT_RGB16F + FSR1_FORMAT_RGB16F_PLANAR; };

// Four adjacent pixels = twelve consecutive elements R0 G0 B0 R1 .. B3 = three four-element accesses.  Element 3 i + c (pixel i,
// channel c) sits in access (3 i + c) / 4 at position (3 i + c) % 4: all compile-time, so unpacking is register selection (8-bit
// codes: one v_cvt_f32_ubyteN per element, no shift-and-mask chain).
template <int FMT>
struct RgbGroup {
  typedef Rgb3<FMT> R;
  typename R::V4 w[3];
  template <int K> __device__ __forceinline__ typename R::E elem() const { return R::template get<K % 4>(w[K / 4]); }
  template <int K> __device__ __forceinline__ void put(typename R::E e) { R::template put<K % 4>(w[K / 4], e); }
  template <int I> __device__ __forceinline__ rgb_t pixel() const {
    return rgb_t{R::load(elem<3 * I>()), R::load(elem<3 * I + 1>()), R::load(elem<3 * I + 2>())};
  }
};

// One pixel, element by element, at address `o` of its R.
template <int FMT>
__device__ __forceinline__ void rgb_store1(char* o, rgbf_t v, bool streaming) {
  typedef typename Rgb3<FMT>::E elem_t;
  store_out<sizeof(elem_t)>(o, Rgb3<FMT>::store(v.r), streaming);
  store_out<sizeof(elem_t)>(o + sizeof(elem_t), Rgb3<FMT>::store(v.g), streaming);
  store_out<sizeof(elem_t)>(o + 2 * sizeof(elem_t), Rgb3<FMT>::store(v.b), streaming);
}

// Lanes of one wave exchange data through LDS: order the wave's own LDS accesses (no other wave touches the region).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The flat run store of an exact-2x EASU tile (WIDE hosts only).  A lane's quad row is two pixels = six elements from an odd pixel
// column: no lane exchange makes that an aligned access.  But a tile row — pixels 64 tx - 1 .. 64 tx + 62 — is 192 elements that
// are CONTIGUOUS in memory, so a wave passes its rows through LDS and writes them as a flat run of aligned four-element stores.
//   * rows start on a four-element boundary (WIDE), so the tile's first element, 3 (64 tx - 1), is element 1 of an aligned group
//     whatever the row: the wave writes tile element e at LDS position e + 1 and the memory groups are the LDS groups.  A lane
//     writes its six elements as element | pair | pair | element (the pairs land on even positions);
//   * a wave filters the two quad rows 2 wave, 2 wave + 1 (its half-waves), i.e. with every call two tile rows of its own: the
//     exchange is wave-local — no workgroup barrier, the footprint stays readable for the other waves — and the buffer (two rows of
//     kRgbRunPitch elements per wave) is a region of its own behind the footprint: 4 x 2 x 196 elements = 6272 B for binary32 on top
//     of the footprint's 12320, which still lets eight workgroups into a CU, the number the waves allow;
//   * lane g < 49 then owns group g of each row: positions 4 g .. 4 g + 3.  Group 0 holds the run's head (three elements; for tx = 0
//     they are column -1: nothing), groups 1 .. 47 the body, group 48 the tail (one element); a group cut by the image's right
//     edge goes element by element, one beyond it or in a row outside the image is not stored.
// `buf`: the wave's buffer; ox0 = 64 tx - 1; row0: the image row of the first half-wave's pixels (the second half-wave's is two
// below).  Every lane of the wave must make the call.
constexpr int kRgbRunPitch = 196;  // 1 + 192 elements, rounded up to whole groups
template <int FMT>
__device__ __forceinline__ void rgb_store_run_rows(typename Rgb3<FMT>::E* buf, int lane, rgbf_t left, rgbf_t right, char* out_frame, long long pitch,
                                                   int ox0, int row0, int W, int H, bool streaming) {
  typedef Rgb3<FMT> R;
  typedef typename R::E elem_t;
  typedef typename R::V4 quad_t;
  typedef typename R::V4 __attribute__((may_alias)) quad_lds_t;  // (the buffer is written as elements and pairs, read as groups)
  typedef typename R::P2 __attribute__((may_alias)) pair_t;
  elem_t* const p = buf + (lane >> 5) * kRgbRunPitch + 6 * (lane & 31) + 1;
  p[0] = R::store(left.r);
  *reinterpret_cast<pair_t*>(p + 1) = R::make2(R::store(left.g), R::store(left.b));
  *reinterpret_cast<pair_t*>(p + 3) = R::make2(R::store(right.r), R::store(right.g));
  p[5] = R::store(right.b);
  wave_lds_sync();
  // valid positions of a row: pixels max(ox0, 0) .. min(ox0 + 63, W - 1)
  const int pa = 3 * (max(ox0, 0) - ox0) + 1, pb = 3 * (min(ox0 + kTileW - 1, W - 1) - ox0) + 3;
  const int p0 = 4 * lane;
  if (p0 <= pb && p0 + 3 >= pa) {  // (lanes 49 .. 63 own nothing: pb <= 192)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int y = row0 + 2 * h;  // wave-uniform
      if (y < 0 || y >= H) continue;
      const quad_t v = *reinterpret_cast<const quad_lds_t*>(buf + h * kRgbRunPitch + p0);
      // position q is image element 3 ox0 + q - 1 of the row
      char* const d = out_frame + (long long)y * pitch + ((long long)(3 * ox0 - 1) + p0) * (long long)sizeof(elem_t);
      if (p0 >= pa && p0 + 3 <= pb) {
        store_out<sizeof(quad_t)>(d, v, streaming);
      } else {
        if (p0 >= pa && p0 <= pb) store_out<sizeof(elem_t)>(d, R::template get<0>(v), streaming);
        if (p0 + 1 >= pa && p0 + 1 <= pb) store_out<sizeof(elem_t)>(d + sizeof(elem_t), R::template get<1>(v), streaming);
        if (p0 + 2 >= pa && p0 + 2 <= pb) store_out<sizeof(elem_t)>(d + 2 * sizeof(elem_t), R::template get<2>(v), streaming);
        if (p0 + 3 >= pa && p0 + 3 <= pb) store_out<sizeof(elem_t)>(d + 3 * sizeof(elem_t), R::template get<3>(v), streaming);
      }
    }
  }
  wave_lds_sync();  // the next call overwrites the buffer
}

}  // namespace fsr1
