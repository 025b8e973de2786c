// Streaming token wire format: ragged packing and byte sessions (l3ac_pack_stream / l3ac_unpack_stream).
//
// bitpack.hip's format, per byte: token t of a stream occupies bits [t * bits, (t + 1) * bits) of a little-endian bit stream, byte k is bits
// [8k, 8k + 8), a stream of n tokens is ceil(n * bits / 8) bytes with its last byte zero-padded.  bitpack.hip's kernels take one rectangle
// whose rows start at bit 0; here every stream of a push has its own length and its own phase:
//   pack:    the stream's VIRTUAL bit string is  held bits (0..7, the low bits of state_in[slot]) ++ take tokens of `bits` bits each;
//            its first `count` bytes go out, its last `keep` bits become state_out[slot];
//   unpack:  held bits (0..bits-1) ++ take bytes; `count` tokens go out, the last `keep` bits become state_out[slot].
// Which byte or token of its stream a push starts at never reaches the device: nothing in a descriptor grows with the age of a stream.
//
// Kernels: blockIdx.y = the stream's descriptor; pack: one thread per output DWORD (it gathers the held bits and the <= 32 / bits + 2 tokens
// that overlap it and stores 4 bytes at once, consecutive lanes consecutive dwords; only a row's last dword, where out_bytes is no multiple
// of 4, is stored byte by byte); unpack: one thread per TOKEN, one dword store each (it reads the <= 5 bytes the token spans with byte loads:
// the rows have any byte alignment and bytes at or after `take` are never read, so no dword load may straddle a row's end; neighbouring
// lanes read neighbouring bytes of the same cache lines).  Every byte / token of a described row below out_bytes / out_tokens is written
// exactly once, zeros after the stream's own.  Thread 0 of a stream's first workgroup writes the next state into the session's OTHER state
// buffer (idle streams included: keep = held copies it), so no launch reads an element that it also writes.
// Shifts: a mask of n bits is formed without 1u << 32, a 64-bit accumulator takes every token / byte at a shift below 32.
// Integer and byte work bound by memory traffic (4 B in, bits / 8 B out per token, and back), exact by construction.
//
// Descriptors are host values passed as kernel arguments, PackStreamBlock::CAP per launch, the ResampleStreamBlock way.
#include <algorithm>
#include <vector>

#include "../kernels.hpp"

namespace {

constexpr int BPS_THREADS = 256;

struct BpsGeom {
    int64_t fresh_stride, out_stride, out_size;  // out_size: out_bytes (pack) / out_tokens (unpack)
    int bits;
};

__host__ __device__ inline uint32_t low_mask(int n) { return n >= 32 ? 0xffffffffu : ((1u << n) - 1u); }  // n in 0..32

// 32 bits of  state[0 : held] ++ src[0 : take] tokens  from bit p on (zeros after the string's end); `state` holds only its held bits
__device__ inline uint32_t pack_string_bits(uint32_t state, int held, const int32_t* __restrict__ src, int take, int bits, int64_t p) {
    const uint32_t mask = low_mask(bits);
    uint64_t acc;
    int filled;
    int64_t t;
    if (p < held) {
        acc = state >> (int)p;
        filled = held - (int)p;
        t = 0;
    } else {
        const int64_t q = p - held;
        t = q / bits;
        if (t >= take) return 0u;
        const int off = (int)(q - t * bits);
        acc = ((uint32_t)src[t] & mask) >> off;
        filled = bits - off;
        ++t;
    }
    for (; filled < 32 && t < take; ++t, filled += bits) acc |= (uint64_t)((uint32_t)src[t] & mask) << filled;  // (shift < 32)
    return (uint32_t)acc;
}

// n <= 32 bits of  state[0 : held] ++ src[0 : take] bytes  from bit p on (zeros after the string's end)
__device__ inline uint32_t unpack_string_bits(uint32_t state, int held, const uint8_t* __restrict__ src, int take, int64_t p, int n) {
    if (n <= 0) return 0u;
    uint64_t acc;
    int filled;
    int64_t k;
    if (p < held) {
        acc = state >> (int)p;
        filled = held - (int)p;
        k = 0;
    } else {
        const int64_t q = p - held;
        k = q >> 3;
        if (k >= take) return 0u;
        const int sh = (int)(q & 7);
        acc = (uint32_t)src[k] >> sh;
        filled = 8 - sh;
        ++k;
    }
    for (; filled < n && k < take; ++k, filled += 8) acc |= (uint64_t)src[k] << filled;  // (shift < 32)
    return (uint32_t)acc & low_mask(n);
}

__global__ __launch_bounds__(BPS_THREADS) void pack_stream_kernel(const uint32_t* __restrict__ state_in, uint32_t* __restrict__ state_out,
                                                                  const int32_t* __restrict__ fresh, uint8_t* __restrict__ out, const BpsGeom g,
                                                                  const PackStreamBlock blk) {
    const l3ac_pack_stream_desc d = blk.desc[blockIdx.y];
    const int32_t* src = fresh + (int64_t)d.slot * g.fresh_stride;  // (not dereferenced when take == 0)
    const uint32_t st = d.held > 0 ? state_in[d.slot] & low_mask(d.held) : 0u;
    const int64_t w = (int64_t)blockIdx.x * BPS_THREADS + threadIdx.x;
    if (w == 0 && state_out)
        state_out[d.slot] = d.keep > 0 ? pack_string_bits(st, d.held, src, d.take, g.bits, (int64_t)8 * d.count) & low_mask(d.keep) : 0u;
    const int64_t b0 = 4 * w;  // this thread's first byte of the row
    if (b0 >= g.out_size) return;
    const int64_t live = (int64_t)d.count - b0;  // bytes of this dword the stream emits; zeros after them
    uint32_t v = 0u;
    if (live > 0) {
        v = pack_string_bits(st, d.held, src, d.take, g.bits, 8 * b0);
        if (live < 4) v &= low_mask(8 * (int)live);  // a stream that goes on keeps the bits of its unfinished byte
    }
    uint8_t* row = out + (int64_t)d.slot * g.out_stride;
    if (b0 + 4 <= g.out_size)
        *reinterpret_cast<uint32_t*>(row + b0) = v;  // rows are 4-byte aligned, out_stride is a multiple of 4
    else
        for (int64_t k = b0; k < g.out_size; ++k) row[k] = (uint8_t)(v >> (8 * (int)(k - b0)));
}

__global__ __launch_bounds__(BPS_THREADS) void unpack_stream_kernel(const uint32_t* __restrict__ state_in, uint32_t* __restrict__ state_out,
                                                                    const uint8_t* __restrict__ fresh, int32_t* __restrict__ out, const BpsGeom g,
                                                                    const UnpackStreamBlock blk) {
    const l3ac_unpack_stream_desc d = blk.desc[blockIdx.y];
    const uint8_t* src = fresh + (int64_t)d.slot * g.fresh_stride;  // (not dereferenced when take == 0)
    const uint32_t st = d.held > 0 ? state_in[d.slot] & low_mask(d.held) : 0u;
    const int64_t t = (int64_t)blockIdx.x * BPS_THREADS + threadIdx.x;
    if (t == 0 && state_out)
        state_out[d.slot] = d.keep > 0 ? unpack_string_bits(st, d.held, src, d.take, (int64_t)d.count * g.bits, d.keep) : 0u;
    if (t >= g.out_size) return;
    out[(int64_t)d.slot * g.out_stride + t] = t < d.count ? (int32_t)unpack_string_bits(st, d.held, src, d.take, t * g.bits, g.bits) : 0;
}

bool bps_apart(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return !a || !b || a0 + (uintptr_t)a_bytes <= b0 || b0 + (uintptr_t)b_bytes <= a0;
}

// what the two entries share: the shapes, the buffers and, per descriptor, the stream and its packet
template <typename Desc>
int bps_check(const char* what, const uint32_t* state_in, uint32_t* state_out, int streams, const void* fresh, int64_t fresh_size,
              int64_t fresh_stride, int fresh_elem, int bits, const Desc* desc, int count, const void* out, int64_t out_size, int64_t out_stride,
              int out_elem) {
    L3AC_REQUIRE(desc && count > 0, "%s: no descriptors", what);
    L3AC_REQUIRE(bits >= 1 && bits <= 32, "%s: %d bits per token outside 1..32", what, bits);
    L3AC_REQUIRE(streams > 0 && fresh_size >= 0 && fresh_size <= INT32_MAX && fresh_stride >= fresh_size && fresh_stride >= 1,
                 "%s: %d streams, %lld new elements in rows of %lld", what, streams, (long long)fresh_size, (long long)fresh_stride);
    L3AC_REQUIRE(out_size >= 0 && out_size <= INT32_MAX && out_stride >= out_size && (out || out_size == 0),
                 "%s: an output of %lld for rows of %lld", what, (long long)out_size, (long long)out_stride);
    const int64_t n_state = (int64_t)streams * 4, n_fresh = (int64_t)streams * fresh_stride * fresh_elem, n_out = (int64_t)streams * out_stride * out_elem;
    L3AC_REQUIRE(!state_in || !state_out || bps_apart(state_in, n_state, state_out, n_state), "%s: the two state buffers overlap", what);
    L3AC_REQUIRE(bps_apart(out, n_out, fresh, n_fresh) && bps_apart(out, n_out, state_in, n_state) && bps_apart(out, n_out, state_out, n_state) &&
                     bps_apart(fresh, n_fresh, state_out, n_state),
                 "%s: the output or the next state overlaps an input", what);
    L3AC_REQUIRE((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out) | reinterpret_cast<uintptr_t>(out)) % 4 == 0,
                 "%s: the state buffers and the output must be 4-byte aligned", what);
    std::vector<int> slots;
    bool carries = false;
    for (int i = 0; i < count; ++i) {
        const Desc& d = desc[i];
        L3AC_REQUIRE(d.slot >= 0 && d.slot < streams, "%s: descriptor %d: stream %d of %d", what, i, d.slot, streams);
        L3AC_REQUIRE(d.take >= 0 && d.take <= fresh_size && (d.take == 0 || fresh), "%s: descriptor %d takes %d of %lld new elements", what, i, d.take,
                     (long long)fresh_size);
        L3AC_REQUIRE(d.count >= 0 && d.count <= out_size, "%s: descriptor %d emits %d into rows of %lld", what, i, d.count, (long long)out_size);
        slots.push_back(d.slot);
        carries = carries || d.held != 0 || d.keep != 0;
    }
    std::sort(slots.begin(), slots.end());
    L3AC_REQUIRE(std::adjacent_find(slots.begin(), slots.end()) == slots.end(), "%s: two descriptors for one stream", what);
    L3AC_REQUIRE(!carries || (state_in && state_out), "%s: a stream holds or keeps bits, but a state buffer is null", what);
    return L3AC_OK;
}

}  // namespace

extern "C" {

int64_t l3ac_packed_bytes(int64_t n_tok, int32_t bits) {
    L3AC_REQUIRE(bits >= 1 && bits <= 32 && n_tok >= 0 && n_tok <= INT64_MAX / 64, "packed_bytes: %lld tokens of %d bits", (long long)n_tok, bits);
    return (n_tok * bits + 7) / 8;
}

int l3ac_pack_stream(const uint32_t* state_in, uint32_t* state_out, int32_t streams, const int32_t* fresh, int64_t fresh_tokens,
                     int64_t fresh_stride, int32_t bits, const l3ac_pack_stream_desc* desc, int32_t count, uint8_t* out, int64_t out_bytes,
                     int64_t out_stride, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_TRY(bps_check("pack_stream", state_in, state_out, streams, fresh, fresh_tokens, fresh_stride, 4, bits, desc, count, out, out_bytes, out_stride, 1));
    L3AC_REQUIRE(out_stride % 4 == 0 && reinterpret_cast<uintptr_t>(fresh) % 4 == 0, "pack_stream: output rows of %lld bytes are no multiple of 4, or "
                 "the tokens are not 4-byte aligned", (long long)out_stride);
    for (int i = 0; i < count; ++i) {
        const l3ac_pack_stream_desc& d = desc[i];
        L3AC_REQUIRE(d.held >= 0 && d.held <= 7, "pack_stream: descriptor %d holds %d bits, outside 0..7", i, d.held);
        const int64_t total = d.held + (int64_t)d.take * bits;  // bits of the virtual string
        L3AC_REQUIRE((d.count == total / 8 && d.keep == total % 8) || (d.count == (total + 7) / 8 && d.keep == 0),
                     "pack_stream: descriptor %d: %d held bits + %d tokens of %d bits give %lld bytes and %lld bits (ended: %lld bytes), not %d and %d", i,
                     d.held, d.take, bits, (long long)(total / 8), (long long)(total % 8), (long long)((total + 7) / 8), d.count, d.keep);
    }
    if (out_bytes == 0 && !state_out) return L3AC_OK;  // nothing to emit, nothing to keep
    BpsGeom g{fresh_stride, out_stride, out_bytes, bits};
    for (int off = 0; off < count; off += PackStreamBlock::CAP) {
        PackStreamBlock blk{};
        const int n = std::min(count - off, (int)PackStreamBlock::CAP);
        double taken = 0.0;
        for (int i = 0; i < n; ++i) {
            blk.desc[i] = desc[off + i];
            taken += blk.desc[i].take;
        }
        const dim3 grid((unsigned)std::max<int64_t>(ceil_div64(ceil_div64(out_bytes, 4), BPS_THREADS), 1), (unsigned)n);
        ProfScope prof(s, "pack_stream_kernel", 0.0, 4.0 * taken + (double)n * out_bytes);
        hipLaunchKernelGGL(pack_stream_kernel, grid, dim3(BPS_THREADS), 0, s, state_in, state_out, fresh, out, g, blk);
        L3AC_LAUNCH_CHECK();
    }
    return L3AC_OK;
}

int l3ac_unpack_stream(const uint32_t* state_in, uint32_t* state_out, int32_t streams, const uint8_t* fresh, int64_t fresh_bytes,
                       int64_t fresh_stride, int32_t bits, const l3ac_unpack_stream_desc* desc, int32_t count, int32_t* out, int64_t out_tokens,
                       int64_t out_stride, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_TRY(bps_check("unpack_stream", state_in, state_out, streams, fresh, fresh_bytes, fresh_stride, 1, bits, desc, count, out, out_tokens, out_stride, 4));
    for (int i = 0; i < count; ++i) {
        const l3ac_unpack_stream_desc& d = desc[i];
        L3AC_REQUIRE(d.held >= 0 && d.held < bits, "unpack_stream: descriptor %d holds %d bits, outside 0..%d", i, d.held, bits - 1);
        const int64_t total = d.held + (int64_t)8 * d.take;  // bits of the virtual string
        const int64_t rest = total - (int64_t)d.count * bits;
        L3AC_REQUIRE((d.count == total / bits && d.keep == total % bits) || (d.keep == 0 && rest >= 0 && rest < std::max(bits, 8)),
                     "unpack_stream: descriptor %d: %d held bits + %d bytes give %lld tokens of %d bits and %lld bits, not %d and %d", i, d.held, d.take,
                     (long long)(total / bits), bits, (long long)(total % bits), d.count, d.keep);
    }
    if (out_tokens == 0 && !state_out) return L3AC_OK;  // nothing to emit, nothing to keep
    BpsGeom g{fresh_stride, out_stride, out_tokens, bits};
    for (int off = 0; off < count; off += UnpackStreamBlock::CAP) {
        UnpackStreamBlock blk{};
        const int n = std::min(count - off, (int)UnpackStreamBlock::CAP);
        double taken = 0.0;
        for (int i = 0; i < n; ++i) {
            blk.desc[i] = desc[off + i];
            taken += blk.desc[i].take;
        }
        const dim3 grid((unsigned)std::max<int64_t>(ceil_div64(out_tokens, BPS_THREADS), 1), (unsigned)n);
        ProfScope prof(s, "unpack_stream_kernel", 0.0, taken + 4.0 * n * out_tokens);
        hipLaunchKernelGGL(unpack_stream_kernel, grid, dim3(BPS_THREADS), 0, s, state_in, state_out, fresh, out, g, blk);
        L3AC_LAUNCH_CHECK();
    }
    return L3AC_OK;
}

}  // extern "C"
