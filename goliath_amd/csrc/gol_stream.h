// gol_stream.h -- what the streaming passes share (optim.hip, regloss.hip; the reduction also imgloss.hip, ssim.hip):
// the global-memory vector types, the chunk geometry and the fixed-order workgroup sum.  Types, constants and the
// reduction only: the per-element loops stay in the kernels.
#pragma once
#include "gol_common.h"

// ---- the fixed-order workgroup sum ----------------------------------------------------------------------------------------
// First half: the DPP ladder over each wave (gol_wave_sum_to_lane63, float or double), lane 63 of wave w writes sh[w],
// barrier.  Every thread may then read sh[0 .. waves).
template <typename T>
__device__ __forceinline__ void gol_wave_sums_to_lds(T v, T* sh) {
  v = gol_wave_sum_to_lane63(v);
  if ((threadIdx.x & (GOL_WAVE - 1)) == GOL_WAVE - 1) sh[threadIdx.x / GOL_WAVE] = v;
  __syncthreads();
}

// Sum over a workgroup of WAVES waves: the ladder, then thread 0 adds the waves in ascending order.  The result is valid in
// thread 0.  The trailing barrier lets the caller hand the same sh[WAVES] to the next sum.
template <typename T, int WAVES>
__device__ __forceinline__ T gol_block_sum(T v, T* sh) {
  gol_wave_sums_to_lds(v, sh);
  T t = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t += sh[w];
  }
  __syncthreads();
  return t;
}

// ---- a chunked pass over flat float arrays: opened with `using namespace gol_stream;` ------------------------------------
namespace gol_stream {

// The tensors are global memory, reached through a 64-bit address from a table or a plain pointer; telling the compiler so
// gives global_load / global_store (an address of unknown space costs a flat access and a wait on both counters).
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f4 gf4;
__device__ __forceinline__ gfloat* global_floats(int64_t addr, int64_t off) {
  return reinterpret_cast<gfloat*>(static_cast<uintptr_t>(addr)) + off;
}
__device__ __forceinline__ const gfloat* global_in(const float* p) {
  return reinterpret_cast<const gfloat*>(reinterpret_cast<uintptr_t>(p));
}
__device__ __forceinline__ gfloat* global_out(float* p) { return reinterpret_cast<gfloat*>(reinterpret_cast<uintptr_t>(p)); }

// One 256-lane workgroup per chunk of 4096 floats = 4 float4 per lane and array; a lane issues all of its 16-byte loads
// before the first use.
constexpr int kBlock = 256;
constexpr int kChunk = 4096;
constexpr int kVecIters = kChunk / 4 / kBlock;   // float4 loads per lane and array

// elements of a chunk when `rem` >= 0 are left from its first one to the end of the array: min(rem, kChunk)
__device__ __forceinline__ int chunk_elems(int64_t rem) { return rem >= kChunk ? kChunk : (int)rem; }

}  // namespace gol_stream
