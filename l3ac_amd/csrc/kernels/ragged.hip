// Per-clip bounds of a ragged batch (l3ac_encode_ragged / l3ac_decode_ragged).
//
// A ragged batch runs on the frame grid of its longest possible clip: clip b's frames at a stage are n[b] * mult of the
// stage's `frames`, the rest of its rows is padding.  These kernels keep the padding from reaching a clip's own frames:
//   ragged_upload_kernel   per-clip counts from the host, as KERNEL ARGUMENTS (a graph replays the values it captured; the
//                          caller's array may change right after the call)
//   ragged_mask_kernel     zeroes the `width` rows after each clip's last frame ([B][N][C]): the zero padding an op that reads
//                          neighbouring frames sees in the clip alone (snake(0) = 0 keeps it zero through the activations)
//   ragged_dup_kernel      copies each clip's last frame into the row after it: linear upsampling then clamps at the clip's
//                          own last frame (ATen i1 = min(i0 + 1, n - 1)) with the arithmetic of the clamped form
//   ragged_gather_kernel   copies clips perm[k0 ..] to / from a compact [count][rows][C] buffer (the LocalTrans split)
#include <algorithm>

#include "../kernels.hpp"

namespace {

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void ragged_upload_kernel(int* __restrict__ dst, const RaggedUpload blk) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i < blk.n) dst[blk.offset + i] = blk.vals[i];
}

// grid (strip blocks, batch): block x of clip b zeroes elements x * THREADS + tid, + gridDim.x * THREADS, ... of the clip's strip
__global__ __launch_bounds__(THREADS) void ragged_mask_kernel(float* __restrict__ x, int frames, int c, const int* __restrict__ n,
                                                             int mult, int width) {
    const int b = blockIdx.y;
    const int64_t first = (int64_t)n[b] * mult;
    const int64_t last = first + width < frames ? first + width : frames;
    if (first >= last) return;
    float* clip = x + ((int64_t)b * frames + first) * c;
    const int64_t count = (last - first) * c;
    for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < count; e += (int64_t)gridDim.x * THREADS) clip[e] = 0.f;
}

__global__ __launch_bounds__(THREADS) void ragged_dup_kernel(float* __restrict__ x, int frames, int c, const int* __restrict__ n,
                                                            int mult) {
    const int b = blockIdx.y;
    const int64_t last = (int64_t)n[b] * mult;  // the row after the clip's last frame
    if (last >= frames || last < 1) return;
    float* row = x + ((int64_t)b * frames + last) * c;
    for (int e = blockIdx.x * THREADS + threadIdx.x; e < c; e += gridDim.x * THREADS) row[e] = row[e - c];
}

// grid (row blocks, count): compact clip k <-> batch clip perm[k0 + k], `rows` rows of c floats (c % 4 == 0)
__global__ __launch_bounds__(THREADS) void ragged_gather_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                               const int* __restrict__ perm, int k0, int rows, int c,
                                                               int64_t batch_clip, int64_t compact_clip, int scatter) {
    const int k = blockIdx.y;
    const int64_t b = perm[k0 + k];
    const float4* s = reinterpret_cast<const float4*>(src + (scatter ? k * compact_clip : b * batch_clip));
    float4* d = reinterpret_cast<float4*>(dst + (scatter ? b * batch_clip : k * compact_clip));
    const int64_t count = (int64_t)rows * c / 4;
    for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < count; e += (int64_t)gridDim.x * THREADS) d[e] = s[e];
}

}  // namespace

int launch_ragged_upload(hipStream_t s, int* dst, const int* host, int n) {
    for (int off = 0; off < n; off += RaggedUpload::CAP) {
        RaggedUpload blk{};
        blk.offset = off;
        blk.n = n - off < RaggedUpload::CAP ? n - off : RaggedUpload::CAP;
        for (int i = 0; i < blk.n; ++i) blk.vals[i] = host[off + i];
        ProfScope prof(s, "ragged_upload_kernel", 0.0, 4.0 * blk.n);
        hipLaunchKernelGGL(ragged_upload_kernel, dim3((unsigned)ceil_div64(blk.n, THREADS)), dim3(THREADS), 0, s, dst, blk);
        L3AC_LAUNCH_CHECK();
    }
    return L3AC_OK;
}

int launch_ragged_mask(hipStream_t s, float* x, int batch, int frames, int c, const int* n, int mult, int width) {
    L3AC_REQUIRE(batch > 0 && batch <= 65535 && frames > 0 && c > 0 && mult > 0 && width > 0, "ragged_mask: bad shape");
    const int64_t strip = (int64_t)std::min(width, frames) * c;
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div64(strip, THREADS), 64);
    ProfScope prof(s, "ragged_mask_kernel", 0.0, 4.0 * (double)strip * batch);
    hipLaunchKernelGGL(ragged_mask_kernel, dim3(blocks, (unsigned)batch), dim3(THREADS), 0, s, x, frames, c, n, mult, width);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int launch_ragged_dup(hipStream_t s, float* x, int batch, int frames, int c, const int* n, int mult) {
    L3AC_REQUIRE(batch > 0 && batch <= 65535 && frames > 0 && c > 0 && mult > 0, "ragged_dup: bad shape");
    ProfScope prof(s, "ragged_dup_kernel", 0.0, 8.0 * (double)c * batch);
    hipLaunchKernelGGL(ragged_dup_kernel, dim3((unsigned)ceil_div64(c, THREADS), (unsigned)batch), dim3(THREADS), 0, s, x, frames, c, n,
                       mult);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int launch_ragged_gather(hipStream_t s, const float* src, float* dst, const int* perm, int k0, int count, int rows, int c,
                         int64_t batch_clip, int64_t compact_clip, bool scatter) {
    L3AC_REQUIRE(count > 0 && count <= 65535 && rows > 0 && c % 4 == 0, "ragged_gather: bad shape");
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div64((int64_t)rows * c / 4, THREADS), 64);
    ProfScope prof(s, "ragged_gather_kernel", 0.0, 8.0 * (double)rows * c * count);
    hipLaunchKernelGGL(ragged_gather_kernel, dim3(blocks, (unsigned)count), dim3(THREADS), 0, s, src, dst, perm, k0, rows, c, batch_clip,
                       compact_clip, scatter ? 1 : 0);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}
