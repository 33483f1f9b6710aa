// RCAS on planar RGB images (FSR1_FORMAT_RGB16F_PLANAR / RGB32F_PLANAR / RGB8_UNORM_PLANAR): a strip kernel of its own, no LDS, no barrier.
//
// RCAS is the pass that is bound by its bytes, and an interleaved RGBA16F pixel carries a quarter of them as
// an alpha that is read and written as 1: three planes move 12 B per pixel where RGBA16F moves 16.
// The strip walk — 256-column waves, four columns per lane, DPP wave shifts, the apron on lanes 0 / 63, the register ring — is
// fsr1_rcas_planar_kernel.h's, shared with the NV12 store of fsr1_rcas_nv12.hip; this file holds what becomes of a finished row here:
//   * per row and plane one store of the load's width (8 bytes fp16, 16 bytes fp32); 8-bit planes: the four results of a plane are
//     encoded and merged into one DWORD before the store: 3 B in and 3 B out per pixel where RGBA8 moves 4 + 4;
//   * WIDE = false — base, pitch, plane or frame stride not a multiple of the four-element access (a tightly packed odd width) —
//     moves every element by itself: no access is ever wider than its alignment.
#include "fsr1_rcas_planar_kernel.h"

namespace fsr1 {

// The plane stores: the strip walk's SINK (fsr1_rcas_planar_kernel.h) of the kernels whose output has the input's format.
template <int FMT, bool WIDE>
struct RcasPlaneStore {
  typedef typename Plane<FMT>::E elem_t;
  typedef typename Plane<FMT>::V4 quad_t;
  typedef Plane<FMT> P;
  const RcasArgs& a;
  const long long ops;
  char* const out_frame;
  const bool stream;
  __device__ __forceinline__ RcasPlaneStore(const RcasArgs& args, int frame)
      : a(args), ops(plane_stride(args.out)), out_frame(args.out.base + (long long)frame * args.out.frame_stride),
        stream((args.flags & FSR1_FLAG_OUTPUT_STREAMING) != 0) {}
  template <bool INTERIOR, bool UP>
  __device__ __forceinline__ void row(int, int y, int, uint32_t off, const bool (&ok)[4], rgb_t o0, rgb_t o1, rgb_t o2, rgb_t o3) const {
    const float out[3][4] = {{o0.r, o1.r, o2.r, o3.r}, {o0.g, o1.g, o2.g, o3.g}, {o0.b, o1.b, o2.b, o3.b}};
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      char* const dst = out_frame + p * ops + (long long)y * a.out.pitch + rcas_planar_zext(off);
      if (WIDE && ok[3]) {
        store_out<sizeof(quad_t)>(dst, P::store4(out[p][0], out[p][1], out[p][2], out[p][3]), stream);
      } else {
        if (ok[0]) store_out<sizeof(elem_t)>(dst, P::store(out[p][0]), stream);
        if (ok[1]) store_out<sizeof(elem_t)>(dst + sizeof(elem_t), P::store(out[p][1]), stream);
        if (ok[2]) store_out<sizeof(elem_t)>(dst + 2 * sizeof(elem_t), P::store(out[p][2]), stream);
        if (ok[3]) store_out<sizeof(elem_t)>(dst + 3 * sizeof(elem_t), P::store(out[p][3]), stream);
      }
    }
  }
};

// OPTS = false: the plain pass (no denoise / HDR square), flags compiled out.  RING: raw rows in flight per lane.
template <int FMT, bool EXACT, bool OPTS, bool WIDE, int RING>
__global__ void __launch_bounds__(kRcasPlanarThreads) rcas_planar_kernel(const RcasArgs a) {
  rcas_planar_workgroup<FMT, EXACT, OPTS, WIDE, RING, RcasPlaneStore<FMT, WIDE>>(a);
}

// Strip height by fsr1_rcas.hip's rule on this kernel's 256-column waves: 16 rows unless that leaves fewer than four waves per SIMD
// (and the launch does not run beside other frames' launches), then 8.
void rcas_planar_geometry(int width, int height, int frames, bool overlapped, int* tiles_x, int* tiles_y, int* rows) {
  const int tx = (width + kRcasPlanarCols - 1) / kRcasPlanarCols;
  int r = 16;
  if (!overlapped && (long long)tx * ((height + r - 1) / r) * frames * kRcasPlanarWaves < 4LL * 4 * 256) r = 8;
  *rows = r;
  *tiles_x = tx;
  *tiles_y = (height + r - 1) / r;
}

// RING by the launch (rcas_planar_shallow_ring).
template <int FMT, bool EXACT, bool OPTS, bool WIDE>
static void rcas_planar_launch_one(const RcasArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kRcasPlanarThreads);
  if constexpr (FMT != FSR1_FORMAT_RGB8_UNORM_PLANAR) {
    if (rcas_planar_shallow_ring(a, FMT)) {
      hipLaunchKernelGGL((rcas_planar_kernel<FMT, EXACT, OPTS, WIDE, 2>), grid, block, 0, stream, a);
      return;
    }
  }
  hipLaunchKernelGGL((rcas_planar_kernel<FMT, EXACT, OPTS, WIDE, 4>), grid, block, 0, stream, a);
}

// wide: the four-element accesses (the host has checked both images' base, pitch, plane and frame stride against them).
hipError_t rcas_planar_launch(const RcasArgs& a, int fmt, bool exact, bool wide, hipStream_t stream) {
  const bool opts = (a.flags & (FSR1_FLAG_RCAS_DENOISE | FSR1_FLAG_HDR_SQUARE)) != 0;
#define FSR1_RCASP(F, E, O, V) rcas_planar_launch_one<F, E, O, V>(a, stream)
#define FSR1_RCASP_V(F, E, O) do { if (wide) FSR1_RCASP(F, E, O, true); else FSR1_RCASP(F, E, O, false); } while (0)
#define FSR1_RCASP_O(F, E) do { if (opts) FSR1_RCASP_V(F, E, true); else FSR1_RCASP_V(F, E, false); } while (0)
#define FSR1_RCASP_E(F) do { if (exact) FSR1_RCASP_O(F, true); else FSR1_RCASP_O(F, false); } while (0)
  switch (fmt) {
    case FSR1_FORMAT_RGB16F_PLANAR: FSR1_RCASP_E(FSR1_FORMAT_RGB16F_PLANAR); break;
    case FSR1_FORMAT_RGB32F_PLANAR: FSR1_RCASP_E(FSR1_FORMAT_RGB32F_PLANAR); break;
    case FSR1_FORMAT_RGB8_UNORM_PLANAR: FSR1_RCASP_E(FSR1_FORMAT_RGB8_UNORM_PLANAR); break;
    default: return hipErrorInvalidValue;
  }
#undef FSR1_RCASP_E
#undef FSR1_RCASP_O
#undef FSR1_RCASP_V
#undef FSR1_RCASP
  return hipGetLastError();
}

}  // namespace fsr1
