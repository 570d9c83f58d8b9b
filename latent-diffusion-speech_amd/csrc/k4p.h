// K4P: the k-interleaved, padded activation layout used between the UNet's kernels.
//
//   tensor [B][C][T] (C % 8 == 0)  ->  [B][C/8][2][T+2][4]
//   channel c = 8q + 2j + h, frame t  ->  ((((b*(C/8) + q)*2 + h)*(T+2) + (t+1))*4 + j
//
// * v_mfma_f32_32x32x2_f32 wants, per lane, ONE scalar of A/B whose k index is 2*kp + (lane>>5).  With this
//   layout the 4 floats at one (row, frame) are the operands of four consecutive MFMAs for lane half h, so an
//   LDS copy of a row segment serves ds_read_b128 operand loads with no transpose and no VALU.
// * frames -1 and T of every row are zero: they are the k3 convolutions' padding, so activation tiles are pure
//   linear copies (LDS-DMA).  Every kernel that writes a K4P tensor also writes its two pad frames.
// * channel concatenation = concatenation of 8-channel blocks, so the UNet's skip-concat is a second base pointer.
#pragma once
#include <hip/hip_runtime.h>

namespace lds {

__host__ __device__ inline long long k4p_index(int C, int T, int b, int c, int t) {
    return ((((long long)b * (C >> 3) + (c >> 3)) * 2 + (c & 1)) * (T + 2) + (t + 1)) * 4 + ((c & 7) >> 1);
}
__host__ __device__ inline long long k4p_floats(int B, int C, int T) { return (long long)B * C * (T + 2); }

// 8-byte write-through store (global_store_dwordx2 ... sc1): the line goes to memory while the kernel is still computing
// instead of staying dirty in the XCD's L2 until the end-of-kernel write-back, which the next launch has to wait for
// (MI355X_MICROARCH.md price list, row "boundary": + bytes / 6 TB/s when the predecessor leaves dirty lines).  Every 64-byte
// line of a K4P row is written whole by one wave instruction (lanes = consecutive frames, both lane halves fill an entry).
typedef float k4p_f32x2 __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ void k4p_store_wt(float* p, k4p_f32x2 v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 16-byte write-through stores of a 32 x 32 MFMA tile (v_mfma_f32_32x32x2_f32: lane = column c + 32 h, register 4g + k = row 8g + 4h + k).
// Register pairs (4g + hh, 4g + 2 + hh) of a lane are elements (2h, 2h + 1) of the entry of row (q0 + g, hh): each lane half holds
// half of BOTH rows' entries, which makes 8-byte stores (one fabric write each when write-through: 2.7x the 16-byte time per byte).
// Two v_permlane32_swap per 8-channel block trade the halves, so that lane half h holds the whole entry of row (q0 + g, hh = h):
//   swap(r0, r1): r0 = {own r0 | lower's r1}, r1 = {upper's r0 | own r1}      (lanes 0-31 | lanes 32-63)
//   swap(r2, r3): r2 = {own r2 | lower's r3}, r3 = {upper's r2 | own r3}      -> entry = (r0, r2, r1, r3)
// Pure data movement: the values stored are bit for bit those of the 8-byte form.  The swaps exchange registers between lanes L and
// L + 32, so k4p_tile_entries must run with ALL lanes active (outside any `if (frame < T)`); the stores may then be predicated.
typedef float k4p_f32x4 __attribute__((ext_vector_type(4)));
typedef float k4p_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned k4p_u32x4 __attribute__((ext_vector_type(4)));
static __device__ __forceinline__ void k4p_tile_entries(const k4p_f32x16& acc, k4p_f32x4 (&e)[4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        // (element copies first: __builtin_bit_cast applied to a vector-element expression reads element 0 of the vector)
        const float r0 = acc[4 * g], r1 = acc[4 * g + 1], r2 = acc[4 * g + 2], r3 = acc[4 * g + 3];
        const auto s01 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, r0), __builtin_bit_cast(unsigned, r1), false, false);
        const auto s23 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, r2), __builtin_bit_cast(unsigned, r3), false, false);
        const unsigned u0 = s01[0], u1 = s23[0], u2 = s01[1], u3 = s23[1];
        e[g] = k4p_f32x4{__builtin_bit_cast(float, u0), __builtin_bit_cast(float, u1), __builtin_bit_cast(float, u2), __builtin_bit_cast(float, u3)};
    }
}
// byte offset, inside one batch element's K4P tensor of Tp entries per row, of this lane half's entry of 8-channel block q at entry index e
static __device__ __forceinline__ int k4p_entry_off(int q, int h, int Tp, int e) { return ((q * 2 + h) * Tp + e) * 16; }
// one entry, write-through (buffer_store_dwordx4 ... sc1, the form of gn_stream's stores) / plain (pad frames)
static __device__ __forceinline__ void k4p_store16_wt(__amdgpu_buffer_rsrc_t r, int off, k4p_f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(k4p_u32x4, v), r, off, 0, 16);
}
static __device__ __forceinline__ void k4p_store16(__amdgpu_buffer_rsrc_t r, int off, k4p_f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(k4p_u32x4, v), r, off, 0, 0);
}

// Ragged batches: lens[b] = valid frames of utterance b at the UNet's input resolution (device int32 [B]; nullptr = every utterance has the
// buffer's length T).  Level l of the UNet halves a length l times the way its stride-2 convolutions do.  Frames at and beyond an
// utterance's length hold zeros in every activation tensor -- they are the convolutions' zero padding, exactly as when the utterance
// runs alone -- so every kernel that writes a tensor writes zeros there, and GroupNorm statistics / attention keys stop at the length.
static __device__ __forceinline__ int ragged_len(const int* lens, int b, int lvl, int T) {
    if (!lens) return T;
    int n = lens[b];
    for (int i = 0; i < lvl; ++i) n = (n - 1) / 2 + 1;
    return n < T ? n : T;
}

}  // namespace lds
