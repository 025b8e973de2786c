// bf16x3 operand splitting and the MFMA primitives shared by gemm_split*.hip and the fused kernels: the vector types, the
// order of the six plane products (the codec's bit contract), the compile-time loop and the LDS-DMA statements.
//
//   x = x0 + x1 + x2,  x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)   (round to nearest even)
//
// Three 8-bit significands cover the 24-bit fp32 significand, so the split is exact; a product a.w is the six plane
// products a_i.w_j with i + j <= 2 (each exact in fp32, the dropped ones are <= 2^-26 |a.w|) summed smallest first in
// the MFMA's fp32 accumulator.
#pragma once

#include <cstdint>
#include <cstring>
#include <type_traits>

#include <hip/hip_runtime.h>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // (arrays of HIP's uint4 struct are not promoted to registers)
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

template <int N, class F, int I = 0>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, F, I + 1>(static_cast<F&&>(f));
    }
}

// two fp32 -> three packed bf16 pairs (low half = first value)
__device__ __forceinline__ void split2(float x0, float x1, unsigned& p0, unsigned& p1, unsigned& p2) {
    const f32x2_t v = {x0, x1};
    p0 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
    const f32x2_t r = {x0 - __builtin_bit_cast(float, p0 << 16), x1 - __builtin_bit_cast(float, p0 & 0xffff0000u)};
    p1 = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2_t));
    const f32x2_t q = {r.x - __builtin_bit_cast(float, p1 << 16), r.y - __builtin_bit_cast(float, p1 & 0xffff0000u)};
    p2 = __builtin_bit_cast(unsigned, __builtin_convertvector(q, bf16x2_t));
}

// The order of the six plane products a[SPLIT_PA[m]] . b[SPLIT_PB[m]], m = 0 .. 5: every kernel form sums them in this order into
// the MFMA's fp32 accumulator, which is what makes the forms agree bit for bit
constexpr int SPLIT_PA[6] = {2, 1, 0, 1, 0, 0}, SPLIT_PB[6] = {0, 1, 2, 0, 1, 0};
constexpr bool split_order_ok() {  // exactly the six pairs with i + j <= 2, each once, i + j non-increasing: "smallest first"
    bool seen[3][3] = {};
    for (int m = 0; m < 6; ++m) {
        const int i = SPLIT_PA[m], j = SPLIT_PB[m];
        if (i < 0 || j < 0 || i + j > 2 || seen[i][j]) return false;
        if (m > 0 && i + j > SPLIT_PA[m - 1] + SPLIT_PB[m - 1]) return false;
        seen[i][j] = true;
    }
    return true;
}
static_assert(split_order_ok(), "SPLIT_PA / SPLIT_PB: the six plane pairs with i + j <= 2, each once, smallest first");

// one of the six plane products of a fragment pair on v_mfma_f32_16x16x32_bf16: D[16 x 16] += A[16 x 32] B[32 x 16]; A: lane
// (row = lane & 15, k group = lane >> 4) holds 8 k values; B: lane (column = lane & 15, k group); D: lane (column = lane & 15),
// registers = rows 4 (lane >> 4) .. + 3.  (Why this shape: DESIGN.md 3.1, 'MFMA shape'.)  A, B: bf16x8, or u32x4 as split2 packs it.
template <int M, class A, class B>
__device__ __forceinline__ f32x4_t mfma_plane(const A (&a)[3], const B (&b)[3], f32x4_t acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[SPLIT_PA[M]]), __builtin_bit_cast(bf16x8, b[SPLIT_PB[M]]), acc, 0, 0, 0);
}
// the same with the product's index in a variable (of a loop that is unrolled)
template <class A, class B>
__device__ __forceinline__ f32x4_t mfma_plane(int m, const A (&a)[3], const B (&b)[3], f32x4_t acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[SPLIT_PA[m]]), __builtin_bit_cast(bf16x8, b[SPLIT_PB[m]]), acc, 0, 0, 0);
}
// acc += a . b over one k step of 32, operands given as their three planes (index = plane)
template <class A, class B>
__device__ __forceinline__ f32x4_t mfma6(const A (&a)[3], const B (&b)[3], f32x4_t acc) {
#pragma unroll
    for (int m = 0; m < 6; ++m) acc = mfma_plane(m, a, b, acc);
    return acc;
}
// the same over one k step of 16 on v_mfma_f32_32x32x16_bf16
__device__ __forceinline__ f32x16_t mfma_split(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16_t acc) {
#pragma unroll
    for (int m = 0; m < 6; ++m) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[SPLIT_PA[m]], b[SPLIT_PB[m]], acc, 0, 0, 0);
    return acc;
}

// A 32 x 32 fp32 accumulator tile X (column on the lane, rows (r&3) + 8(r>>2) + 4h in the 16 registers) as the B operand
// of the next 32x32x16 products, Y = W . X summed over X's ROWS: registers 8s..8s+7 become k step s, whose element j in
// lane half h is row 16s + 8(j>>2) + 4h + (j&3) of X — the other operand's fragments must use the same k order
// (SIGMA below; guide §3 "An accumulator tile as the next MFMA's operand").
__device__ __forceinline__ void split_acc_tile(const f32x16_t& x, bf16x8 (&out)[2][3]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        unsigned p[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) split2(x[8 * s + 2 * j], x[8 * s + 2 * j + 1], p[0][j], p[1][j], p[2][j]);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) out[s][pl] = __builtin_bit_cast(bf16x8, u32x4{p[pl][0], p[pl][1], p[pl][2], p[pl][3]});
    }
}
__host__ __device__ inline int split_sigma(int s, int h, int j) { return 16 * s + 8 * (j >> 2) + 4 * h + (j & 3); }
// the row of accumulator register r in lane half hh of a 32 x 32 tile
__device__ __forceinline__ int split_rowmap(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// this wave's quarter of one ring slot: N 1-KB LDS-DMA pieces, lane l copying 16 B from base + 16 l + 1024 i to lds_dst + 16 l + 1024 i.
// One statement = one M0 write for all pieces (the instruction offset is added to the global AND the LDS address; both are
// passed pre-biased by +3072 when N = 6 so that the offsets fit the signed 13-bit field), a wave-uniform 64-bit base in SGPRs
// and one loop-invariant 32-bit lane offset: no vector address arithmetic per piece (guide 5.7: M0 is written in the statement
// that uses it; the copies are invisible to hipcc's s_waitcnt bookkeeping and are counted by hand).
// NT: non-temporal policy on the copies (aux = nt).  For a stream that ONE workgroup per XCD or so reads once from beyond L2 (the
// half-tile form: a single clip) the copies land sooner (guide, price list 'nt-weights'); never for the batch form, whose 256
// workgroups re-read the image from L2 in step.
template <int N, bool NT = false>
__device__ __forceinline__ void dma_slot_quarter(const unsigned char* base, unsigned lane_off, unsigned lds_dst) {
    static_assert(N == 3 || N == 6, "3 KB or 6 KB per wave");
    unsigned keep;
#define L3AC_DMA3(POL)                                                     \
    asm volatile(                                                          \
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"             \
        "global_load_lds_dwordx4 %1, %2" POL "\n\t"                        \
        "global_load_lds_dwordx4 %1, %2 offset:1024" POL "\n\t"            \
        "global_load_lds_dwordx4 %1, %2 offset:2048" POL "\n\t"            \
        "s_mov_b32 m0, %0"                                                 \
        : "=&s"(keep)                                                      \
        : "v"(lane_off), "s"(base), "s"(lds_dst)                           \
        : "memory")
#define L3AC_DMA6(POL)                                                     \
    asm volatile(                                                          \
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"             \
        "global_load_lds_dwordx4 %1, %2 offset:-3072" POL "\n\t"           \
        "global_load_lds_dwordx4 %1, %2 offset:-2048" POL "\n\t"           \
        "global_load_lds_dwordx4 %1, %2 offset:-1024" POL "\n\t"           \
        "global_load_lds_dwordx4 %1, %2" POL "\n\t"                        \
        "global_load_lds_dwordx4 %1, %2 offset:1024" POL "\n\t"            \
        "global_load_lds_dwordx4 %1, %2 offset:2048" POL "\n\t"            \
        "s_mov_b32 m0, %0"                                                 \
        : "=&s"(keep)                                                      \
        : "v"(lane_off), "s"(base + 3072), "s"(lds_dst + 3072u)            \
        : "memory")
    if constexpr (N == 3) {
        if constexpr (NT) L3AC_DMA3(" nt"); else L3AC_DMA3("");
    } else {
        if constexpr (NT) L3AC_DMA6(" nt"); else L3AC_DMA6("");
    }
#undef L3AC_DMA3
#undef L3AC_DMA6
}

// one 1-KB block (lane l copies 16 B from base + 16 l to lds_dst + 16 l)
__device__ __forceinline__ void dma_1k(const unsigned char* base, unsigned lane_off, unsigned lds_dst) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(lane_off), "s"(base), "s"(lds_dst)
        : "memory");
}

// host side (weights are finite)
inline uint16_t bf16_rne_host(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_to_f32_host(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
inline void split3_host(float x, uint16_t (&out)[3]) {
    out[0] = bf16_rne_host(x);
    const float r1 = x - bf16_to_f32_host(out[0]);
    out[1] = bf16_rne_host(r1);
    out[2] = bf16_rne_host(r1 - bf16_to_f32_host(out[1]));
}
