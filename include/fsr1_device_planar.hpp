// Planar RGB storage (FSR1_FORMAT_RGB16F_PLANAR / RGB32F_PLANAR / RGB8_UNORM_PLANAR) for the tiled forms: three planes R, G, B of
// `height` rows each, rows `pitch` bytes apart, plane p of a frame at frame + p * pitch * height — a contiguous (N,3,H,W)
// tensor, or one whose rows are padded.  The filters are the ones of fsr1_device_easu.hpp / fsr1_device_rcas.hpp on the same LDS
// records and registers; what differs is the two ends that touch memory: this header holds the element types, the footprint
// staging of EASU (three coalesced element loads per texel in place of one texel load) and the plane stores.
//
// Every global access is naturally aligned to its own width: a kernel takes a two- or four-element access only where its
// instantiation (WIDE) was chosen by a host that has checked base, pitch, plane and frame stride against that width.
#pragma once
#include "fsr1_device_easu.hpp"
#include "fsr1_device_rcas.hpp"

namespace fsr1 {

// load / store: an element to and from the filter's binary32.  V4: four adjacent columns of a plane row as one access; make4 builds
// it from elements, get<I> reads column I, put<I> replaces it, store4 = make4 of four stored values.
template <int FMT> struct Plane;  // FMT = a planar fsr1_format
template <> struct Plane<FSR1_FORMAT_RGB16F_PLANAR> {
  typedef half_t E;                                                      // one element of a plane
  typedef half_t V2 __attribute__((ext_vector_type(2), aligned(4)));     // two / four adjacent columns of a plane row
  typedef half_t V4 __attribute__((ext_vector_type(4), aligned(8)));
  static __device__ __forceinline__ float load(E e) { return (float)e; }
  static __device__ __forceinline__ E store(float x) { return (half_t)x; }  // RTNE, as Pixel<RGBA16F>::store
  static __device__ __forceinline__ V4 make4(E a, E b, E c, E d) { return V4{a, b, c, d}; }
  template <int I> static __device__ __forceinline__ E get(const V4& v) { return v[I]; }
  template <int I> static __device__ __forceinline__ void put(V4& v, E e) { v[I] = e; }
  static __device__ __forceinline__ V4 store4(float a, float b, float c, float d) { return V4{store(a), store(b), store(c), store(d)}; }
};
template <> struct Plane<FSR1_FORMAT_RGB32F_PLANAR> {
  typedef float E;
  typedef float V2 __attribute__((ext_vector_type(2), aligned(8)));
  typedef float V4 __attribute__((ext_vector_type(4), aligned(16)));
  static __device__ __forceinline__ float load(E e) { return e; }
  static __device__ __forceinline__ E store(float x) { return x; }
  static __device__ __forceinline__ V4 make4(E a, E b, E c, E d) { return V4{a, b, c, d}; }
  template <int I> static __device__ __forceinline__ E get(const V4& v) { return v[I]; }
  template <int I> static __device__ __forceinline__ void put(V4& v, E e) { v[I] = e; }
  static __device__ __forceinline__ V4 store4(float a, float b, float c, float d) { return V4{a, b, c, d}; }
};
// 8-bit UNORM codes under the conversions pinned for RGBA8_UNORM (fsr1_hip.h).  Four columns are ONE dword, column I in byte I: a row
// in flight costs a lane one register per plane, decoding column I is one v_cvt_f32_ubyteI and its two-instruction correction, and
// four results are encoded and merged into the dword before the store.
template <> struct Plane<FSR1_FORMAT_RGB8_UNORM_PLANAR> {
  typedef uint8_t E;
  typedef uint32_t V4;
  static __device__ __forceinline__ float load(E e) { return unorm_decode<255>(e); }
  static __device__ __forceinline__ E store(float x) { return (E)unorm_encode<255>(x); }
  static __device__ __forceinline__ V4 make4(E a, E b, E c, E d) { return (V4)a | ((V4)b << 8) | ((V4)c << 16) | ((V4)d << 24); }
  template <int I> static __device__ __forceinline__ E get(const V4& v) { return (E)(v >> (8 * I)); }
  template <int I> static __device__ __forceinline__ void put(V4& v, E e) { v = (v & ~(0xffu << (8 * I))) | ((V4)e << (8 * I)); }
  static __device__ __forceinline__ V4 store4(float a, float b, float c, float d) {  // (codes are <= 255: nothing to mask)
    return unorm_encode<255>(a) | (unorm_encode<255>(b) << 8) | (unorm_encode<255>(c) << 16) | (unorm_encode<255>(d) << 24);
  }
};

// bytes between the planes of a frame
__device__ __forceinline__ long long plane_stride(const ImageView& v) { return v.pitch * (long long)v.height; }

// Phase 2 of easu_stage_footprint on the dense LDS layout, behind the barrier that ends a phase 1: FsrEasuSetF's terms for columns
// 1 .. fw - 2, rows 1 .. fh - 2 of the footprint.  Shared by the stagings that differ in phase 1 only (planes here, NV12 in
// fsr1_device_nv12.hpp).  FW: compile-time footprint width, 0 = run-time.  Ends with a barrier.
template <bool EXACT, int FW, int THREADS>
__device__ __forceinline__ void easu_stage_analysis(const EasuLds& l, int fw, int fh, int tid) {
  __syncthreads();
  const int iw = fw - 2, m = iw * (fh - 2);
  const float inv_iw = __builtin_amdgcn_rcpf((float)iw);
  const float* const lum = reinterpret_cast<const float*>(l.tex) + 3;
  for (int j = tid; j < m; j += THREADS) {
    const int y = FW ? j / (FW - 2) : (int)(((float)j + 0.5f) * inv_iw);
    const int i = (y + 1) * fw + (j - y * iw) + 1;
    l.ana[i] = easu_analysis<EXACT>(lum[4 * (i - fw)], lum[4 * (i - 1)], lum[4 * i], lum[4 * (i + 1)], lum[4 * (i + fw)]);
  }
  __syncthreads();
}

// Phases 1 and 2 of easu_stage_footprint for a planar input: the same LDS records (R, G, B, luma*2 | analysis) for the footprint
// [fx0, fx0 + fw) x [fy0, fy0 + fh) with the sampler's clamp-to-edge applied, so phase 3 runs unchanged.  One wave per footprint
// row, one lane per footprint column: the three plane-row bases are scalar, a lane reads its (clamped) column from each plane,
// and a wave issues the loads of all the rows of a trip before it converts the first.  Ends with a barrier.
// FW, FH: compile-time footprint extent (the exact-2x tiles), 0 = run-time.  Footprints wider than a wave (minification) take a
// linear walk.  All THREADS threads of the workgroup must make the call.
// PX: elements from one texel to the next in a row — 1 for planes; 3 for the packed 3-channel images of fsr1_device_rgb.hpp, whose
// channels are then one element apart instead of a plane.
template <int FMT, bool EXACT, int FW = 0, int FH = 0, int THREADS = 256, int PX = 1>
__device__ __forceinline__ void easu_stage_footprint_planar(const EasuLds& l, const ImageView& in, const char* in_frame, int fx0, int fy0,
                                                            int fw_rt, int fh_rt, int tid) {
  typedef typename Plane<FMT>::E elem_t;
  const int fw = FW ? FW : fw_rt, fh = FH ? FH : fh_rt;
  const long long ps = PX == 1 ? plane_stride(in) : (long long)sizeof(elem_t);
  auto record = [](elem_t r, elem_t g, elem_t b) {
    const float fr = Plane<FMT>::load(r), fg = Plane<FMT>::load(g), fb = Plane<FMT>::load(b);
    return float4_t{fr, fg, fb, fmaf(fb, 0.5f, fmaf(fr, 0.5f, fg))};  // :363-366, as easu_stage_footprint
  };
  if (FW || fw <= 64) {
    static_assert(FW <= 64 && THREADS % 64 == 0, "one lane per footprint column");
    constexpr int kWaves = THREADS / 64;
    constexpr int kU = FH ? (FH + kWaves - 1) / kWaves : 5;  // rows per wave and trip: 3 kU element loads in flight per lane
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t xoff = (uint32_t)min(max(fx0 + lane, 0), in.width - 1) * (uint32_t)(PX * sizeof(elem_t));
    float4_t* const rec = l.tex + lane;
    if (lane < fw) {
#pragma unroll 1
      for (int ly0 = wave; ly0 < fh; ly0 += kWaves * kU) {
        elem_t px[kU][3];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int ly = ly0 + kWaves * u;  // wave-uniform
          if (ly < fh) {
            const char* const row = in_frame + (long long)min(max(fy0 + ly, 0), in.height - 1) * in.pitch;
#pragma unroll
            for (int c = 0; c < 3; ++c) px[u][c] = *reinterpret_cast<const elem_t*>(row + c * ps + (size_t)xoff);
          }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int ly = ly0 + kWaves * u;
          if (ly < fh) rec[ly * fw] = record(px[u][0], px[u][1], px[u][2]);
        }
      }
    }
  } else {
    const int n = fw * fh;
    const float inv_fw = __builtin_amdgcn_rcpf((float)fw);  // (i + 0.5) / fw lies 0.5 / fw from an integer: 1 ulp is plenty
    for (int i = tid; i < n; i += THREADS) {
      const int ly = (int)(((float)i + 0.5f) * inv_fw);
      const int gy = min(max(fy0 + ly, 0), in.height - 1), gx = min(max(fx0 + (i - ly * fw), 0), in.width - 1);
      const char* const p = in_frame + (long long)gy * in.pitch + (size_t)gx * (PX * sizeof(elem_t));
      l.tex[i] = record(*reinterpret_cast<const elem_t*>(p), *reinterpret_cast<const elem_t*>(p + ps), *reinterpret_cast<const elem_t*>(p + 2 * ps));
    }
  }
  easu_stage_analysis<EXACT, FW, THREADS>(l, fw, fh, tid);
}

// One value per plane at column / row address `o` of plane R (`ps` bytes between planes).
template <int FMT>
__device__ __forceinline__ void planar_store1(char* o, long long ps, rgbf_t v, bool streaming) {
  typedef typename Plane<FMT>::E elem_t;
  store_out<sizeof(elem_t)>(o, Plane<FMT>::store(v.r), streaming);
  store_out<sizeof(elem_t)>(o + ps, Plane<FMT>::store(v.g), streaming);
  store_out<sizeof(elem_t)>(o + 2 * ps, Plane<FMT>::store(v.b), streaming);
}
// Two adjacent columns per plane as one access; `o` must be aligned to two elements.
template <int FMT>
__device__ __forceinline__ void planar_store2(char* o, long long ps, rgbf_t v0, rgbf_t v1, bool streaming) {
  typedef typename Plane<FMT>::V2 pair_t;
  store_out<sizeof(pair_t)>(o, pair_t{Plane<FMT>::store(v0.r), Plane<FMT>::store(v1.r)}, streaming);
  store_out<sizeof(pair_t)>(o + ps, pair_t{Plane<FMT>::store(v0.g), Plane<FMT>::store(v1.g)}, streaming);
  store_out<sizeof(pair_t)>(o + 2 * ps, pair_t{Plane<FMT>::store(v0.b), Plane<FMT>::store(v1.b)}, streaming);
}

// A row of an exact-2x quad into the planes.  The quad's columns are {odd, even}: in a plane the lane's own pair is not aligned
// to two elements, so (WIDE) every lane takes the LEFT pixel of the lane to its right (one DPP move per channel) and stores the
// aligned pair {own right pixel, right neighbour's left pixel}; the tile's first quad column stores its left pixel alone and the
// last one its right pixel alone.  Every lane of the wave must make the call (the neighbour's value travels through it);
// `o` = address of the left pixel in plane R, xin0 / xin1: the left / right pixel lies inside the image, xin2: so does the
// right neighbour's left pixel, qx: quad column in the 32-quad tile row.  WIDE = false: the two pixels element by element.
template <int FMT, bool WIDE>
__device__ __forceinline__ void planar_store_quad_row(char* o, long long ps, rgbf_t left, rgbf_t right, int qx, bool row_in, bool xin0, bool xin1,
                                                      bool xin2, bool streaming) {
  typedef typename Plane<FMT>::E elem_t;
  if constexpr (WIDE) {
    const rgbf_t nl = {dpp_f32<kDppWaveShl1>(left.r, left.r), dpp_f32<kDppWaveShl1>(left.g, left.g), dpp_f32<kDppWaveShl1>(left.b, left.b)};
    if (!row_in) return;
    if (qx == 0 && xin0) planar_store1<FMT>(o, ps, left, streaming);
    if (qx < 31 && xin2) planar_store2<FMT>(o + sizeof(elem_t), ps, right, nl, streaming);
    else if (xin1) planar_store1<FMT>(o + sizeof(elem_t), ps, right, streaming);
  } else {
    if (!row_in) return;
    if (xin0) planar_store1<FMT>(o, ps, left, streaming);
    if (xin1) planar_store1<FMT>(o + sizeof(elem_t), ps, right, streaming);
  }
}

// The same row for 8-bit planes, where the aligned pair is only two bytes: the four-column form.  Each lane encodes its two pixels and
// packs the codes (R | G << 8 | B << 16), takes the packed LEFT pixel of the lane to its right (one DPP move for the three channels)
// and so holds its aligned pair {own right, neighbour's left}; two more moves hand the neighbour's pair on, and the EVEN quad columns
// store one dword per plane — columns 64 tx + 2 qx .. + 3 of the row, a multiple of four — while the odd ones store nothing.  Quad
// column 0 also stores its left pixel (the tile's first column) by itself; quad column 30 has only three columns left in the tile (the
// fourth byte it was handed belongs to the next quad row) and stores them, like a dword cut by the image's right edge, byte by byte.
// Every lane of the wave must make the call; `o` = address of the left pixel (column oxa, odd) in plane R, W = image width.
// WIDE = false: the two pixels byte by byte.
__device__ __forceinline__ uint32_t planar_codes(rgbf_t v) { return unorm_encode<255>(v.r) | (unorm_encode<255>(v.g) << 8) | (unorm_encode<255>(v.b) << 16); }
__device__ __forceinline__ uint32_t dpp_shl1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, kDppWaveShl1, 0xf, 0xf, false); }
__device__ __forceinline__ void planar_store_codes(char* o, long long ps, uint32_t codes, bool streaming) {
  store_out<1>(o, (uint8_t)codes, streaming);
  store_out<1>(o + ps, (uint8_t)(codes >> 8), streaming);
  store_out<1>(o + 2 * ps, (uint8_t)(codes >> 16), streaming);
}
template <bool WIDE>
__device__ __forceinline__ void planar_store_quad_row_u8(char* o, long long ps, rgbf_t left, rgbf_t right, int qx, int oxa, int W, bool row_in,
                                                         bool streaming) {
  const uint32_t l = planar_codes(left), r = planar_codes(right);
  if constexpr (WIDE) {
    const uint32_t nl = dpp_shl1(l);                       // own pair = {r, nl}
    const uint32_t nr = dpp_shl1(r), nnl = dpp_shl1(nl);  // the right neighbour's pair
    if (!row_in || (qx & 1)) return;
    if (qx == 0 && oxa >= 0) planar_store_codes(o, ps, l, streaming);
    const int n = min(qx == 30 ? 3 : 4, W - (oxa + 1));  // columns oxa + 1 .. oxa + n are this lane's to store (n <= 0: none)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t quad = ((r >> (8 * c)) & 0xffu) | (((nl >> (8 * c)) & 0xffu) << 8) | (((nr >> (8 * c)) & 0xffu) << 16) | ((nnl >> (8 * c)) << 24);
      char* const p = o + 1 + c * ps;
      if (n == 4) {
        store_out<4>(p, quad, streaming);
      } else {
        if (n > 0) store_out<1>(p, (uint8_t)quad, streaming);
        if (n > 1) store_out<1>(p + 1, (uint8_t)(quad >> 8), streaming);
        if (n > 2) store_out<1>(p + 2, (uint8_t)(quad >> 16), streaming);
      }
    }
  } else {
    if (!row_in) return;
    if (oxa >= 0 && oxa < W) planar_store_codes(o, ps, l, streaming);
    if (oxa + 1 < W) planar_store_codes(o + 1, ps, r, streaming);
  }
}

}  // namespace fsr1
