// gol_splitbf16.h -- what the split-bf16 ("bf16x3") MFMA operators share: conv3x.hip (3x3 / stride 1, VGG19) and conv4x.hip
// (4x4 / stride 2, URHand's FeatEncoderUNet).  An operand v is written as hi = bf16_rne(v), lo = bf16_rne(v - float(hi)) (the
// subtraction is exact in fp32) and a product is lo hi + hi lo + hi hi on v_mfma_f32_16x16x32_bf16, summed in fp32; lo lo is
// dropped.  Here: the vector types, the split of eight values, and the slot swizzle of an LDS image with 64-byte rows (32
// bf16: the K of one MFMA) that is read 16 bytes per lane.  Everything is inline and file-local (anonymous namespace).
#pragma once
#include "gol_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// the 16-byte slot (0..3) of chunk q in row n of an LDS image with 64-byte rows: 16 CONSECUTIVE rows read by the lanes
// (j = lane & 15 -> row base + j, g = lane >> 4 -> chunk g) of a ds_read_b128 hit, in every 16-lane group of that
// instruction ({0-3,12-15,20-27}, ...), 16 distinct slots of the 256-byte bank row, whatever the base
__device__ __forceinline__ int cx_slot(int n, int q) { return q ^ ((n >> 1) & 2); }

// v = hi + lo + O(2^-16 |v|), both bf16 by round to nearest even
__device__ __forceinline__ void cx_split(const f32x8 v, bf16x8& hi, bf16x8& lo) {
  hi = __builtin_convertvector(v, bf16x8);
  lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x8), bf16x8);
}

}  // namespace
