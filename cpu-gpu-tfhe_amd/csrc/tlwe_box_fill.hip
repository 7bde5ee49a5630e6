// tlwe_box_fill.hip — spreads a packed value over its box.
//
// The packing key switch puts value m at ONE coefficient, m w; a blind rotation that starts from the
// packed sample reads the coefficient the selector's phase points at, anywhere in box m = [m w,
// (m + 1) w) of the LUT convention (w = N / p).  Multiplying both polynomials of the sample by
// 1 + X + ... + X^(w - 1) copies the phase at m w to the whole box (and sums the pack's noise at the
// w - 1 unoccupied coefficients before it into each):
//
//   out[j] = sum_{k < w} +- in[(j - k) mod N],  minus where j - k < 0      (negacyclic, exact mod 2^32)
//
// With the inclusive prefix sums S[j] = in[0] + ... + in[j] (S[-1] = 0) that is
//   out[j] = S[j] - S[j - w]                          for j >= w - 1,
//   out[j] = S[j] - (S[N - 1] - S[N + j - w])         for j <  w - 1   (the wrapped part, negated),
// so a polynomial costs one scan instead of w loads per word.  One workgroup of 256 threads per
// polynomial, 4 consecutive words per thread: a serial sum in registers, a scan across the wave's
// lanes, the four wave totals through LDS, then S in LDS for the two reads per output word.  Every
// input word is in LDS before the first output word is written, so out may be in.
#include "engine.h"

namespace tfhe_amd {

namespace {

constexpr int kFillThreads = 256;
static_assert(kFillThreads * 4 == kN, "4 words per thread");

__global__ __launch_bounds__(kFillThreads) void k_tlwe_box_fill(int log_w, const int32_t *in, int32_t *out) {   // (out may be in)
    __shared__ uint32_t S[kN];
    __shared__ uint32_t wave_total[kFillThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t poly = (size_t)blockIdx.x * kN;   // blockIdx.x < 2 T: polynomial c of sample t at (2 t + c) kN
    const int32_t *src = in + poly + 4 * tid;   // (word loads: the caller's arrays need no 16-byte alignment)
    const uint32_t s0 = (uint32_t)src[0], s1 = s0 + (uint32_t)src[1], s2 = s1 + (uint32_t)src[2],
                   s3 = s2 + (uint32_t)src[3];
    uint32_t run = s3;   // inclusive scan of the threads' sums over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)run, d, 64);
        if (lane >= d) run += up;
    }
    if (lane == 63) wave_total[wave] = run;
    __syncthreads();
    uint32_t before = run - s3;   // the words before this thread's four: its wave's lanes, then the waves before
    for (int k = 0; k < wave; ++k) before += wave_total[k];
    S[4 * tid] = before + s0;
    S[4 * tid + 1] = before + s1;
    S[4 * tid + 2] = before + s2;
    S[4 * tid + 3] = before + s3;
    __syncthreads();
    const int w = 1 << log_w;
    const uint32_t total = S[kN - 1];
    uint32_t o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = 4 * tid + r;
        if (j >= w) o[r] = S[j] - S[j - w];
        else if (j == w - 1) o[r] = S[j];
        else o[r] = S[j] - (total - S[kN + j - w]);   // kN + j - w in [kN - w + 0, kN - 2]: inside S
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) out[poly + 4 * tid + r] = (int32_t)o[r];
}

}  // namespace

hipError_t launch_tlwe_box_fill(int T, int log_w, const int32_t *in, int32_t *out, hipStream_t s) {
    if (T <= 0) return hipSuccess;
    if (!in || !out || log_w < 0 || log_w > kLogN || (long)T * 2 > 0x7fffffffL) return hipErrorInvalidValue;
    trace_kernel("k_tlwe_box_fill");
    hipLaunchKernelGGL(k_tlwe_box_fill, dim3(2 * (unsigned)T), dim3(kFillThreads), 0, s, log_w, in, out);
    return hipGetLastError();
}

}  // namespace tfhe_amd
