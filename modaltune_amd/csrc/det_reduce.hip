// Deterministic mode: the ONE reduce kernel behind every launcher's deterministic form (include/modaltune_hip.h, "deterministic forms":
// MtLaunchOpts.partials).  A DET kernel stores its workgroups' partial results with plain stores, each to a slot that is a pure function of blockIdx;
// this kernel then adds them up in ASCENDING slot order -- a fixed association, whatever order the workgroups retired in -- and
// adds the sum to the destination (the `+=` of the atomic forms):
//   dst[r * ldd + c] += ((p[0] + p[1]) + p[2]) + ...     p[i] = partials[i * part_stride + r * cols + c]
// No LDS, no atomics; an element is owned by one thread.  The caller passes only slots that a workgroup wrote.
#include "common.h"

namespace {

template <int V>      // V = 4: 16-byte accesses (cols, ldd, part_stride multiples of 4; both pointers 16-byte aligned); V = 1 otherwise
__global__ __launch_bounds__(256) void det_reduce_kernel(const float* __restrict__ partials, int nparts, int rows, int cols, long part_stride,
                                                         float* __restrict__ dst, long ldd) {
  typedef float vec __attribute__((ext_vector_type(V)));
  const int cv = cols / V;
  const long n = (long)rows * cv;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / cv;
    const int c = (int)(i - r * cv) * V;
    const float* p = partials + r * cols + c;
    vec s = *reinterpret_cast<const vec*>(p);
    int k = 1;
    for (; k + 4 <= nparts; k += 4) {      // four loads in flight, summed in slot order
      const vec a0 = *reinterpret_cast<const vec*>(p + (k + 0) * part_stride);
      const vec a1 = *reinterpret_cast<const vec*>(p + (k + 1) * part_stride);
      const vec a2 = *reinterpret_cast<const vec*>(p + (k + 2) * part_stride);
      const vec a3 = *reinterpret_cast<const vec*>(p + (k + 3) * part_stride);
      s += a0; s += a1; s += a2; s += a3;
    }
    for (; k < nparts; ++k) s += *reinterpret_cast<const vec*>(p + k * part_stride);
    vec* d = reinterpret_cast<vec*>(dst + r * ldd + c);
    *d = *d + s;
  }
}

}  // namespace

int mt_det_reduce_launch(const float* partials, int nparts, int rows, int cols, long part_stride, float* dst, long ldd, hipStream_t s) {
  if (!partials || !dst || nparts < 1 || rows < 1 || cols < 1 || ldd < cols || part_stride < (long)rows * cols) return MT_ERR_BAD_ARG;
  const bool v4 = !(cols & 3) && !(ldd & 3) && !(part_stride & 3) && !((uintptr_t)partials & 15) && !((uintptr_t)dst & 15);
  const long n = (long)rows * (v4 ? cols / 4 : cols);
  const int grid = (int)max(1L, min((n + 255) / 256, 2048L));
  if (v4) hipLaunchKernelGGL(det_reduce_kernel<4>, dim3(grid), dim3(256), 0, s, partials, nparts, rows, cols, part_stride, dst, ldd);
  else hipLaunchKernelGGL(det_reduce_kernel<1>, dim3(grid), dim3(256), 0, s, partials, nparts, rows, cols, part_stride, dst, ldd);
  MT_CHECK_LAUNCH();
  return MT_OK;
}
