// pack_v4.hip — LWE -> TLWE packing key switch (pack.cpp): the public functional key
// switch with f = identity onto coefficient positions, in the exact two-prime NTT arithmetic of the
// v4 blind rotation (ntt_wave.h).
//
//   OUT = (0, sum_p b_p X^pos[p]) - sum_{i < 500, j = 1..6} D_ij (*) K_ij,
//   D_ij = sum_p d_j(a_p[i]) X^pos[p],   K_ij a TLWE encryption of s_i 2^(32 - 4 j)
//
// Two kernels per batch of outputs:
//   k_pack_digits  transposes the masks into the key object's scratch dig [T][500][kN]: word
//                  (i, pos[p]) holds the six 4-bit digits of a_p[i], unoccupied positions the digits
//                  of 0; it also writes (0, sum_p b_p X^pos[p]) into the output
//                  (k_pack_digits_fm: the same pass over function-major inputs [P][T][500] at the
//                  positions p * pos_step, for the p-way selection of DESIGN.md §3.8;
//                  k_pack_digits_rows: the same pass gathering each output's inputs from a circuit's
//                  wire table through a per-row record, for the select rows of DESIGN.md §3.9);
//   k_pack_v4      one workgroup per (output, slice of the 3 000 key rows), two waves, one per
//                  prime: digits -> ntt_fwd<4> -> Montgomery MAC against key group g, summed in the
//                  NTT domain; every kPackChunkUnits units one inverse transform, CRT lift and
//                  reduction mod 2^32 into registers; at the end the slice's partial result is
//                  subtracted from the output (atomically when the rows are split over workgroups:
//                  sums mod 2^32 are exact in any order).
// The key is 750 groups of 4 rows x 2 polynomials in the bootstrapping key's bk_v2 layout (engine.h).
#include "engine.h"
#include "modarith.h"
#include "ntt_wave.h"

namespace tfhe_amd {

namespace {

constexpr int kPackThreads = 128;
// a unit = 12 key rows = the 6 digits of two key bits = 3 key groups of 4 rows: a wave reads the
// digit words of exactly two mask columns per unit and every shift below is a constant
constexpr int kPackChunkUnits = 21;
// Exactness: one row's product has |c| <= 1024 * 8 * 2^31 = 2^44 and the centred CRT lift is exact
// for |c| < 2^52 (params.h), so at most 256 rows (64 groups) may be summed in the NTT domain before
// the inverse transform and the lift; a chunk is 21 units = 63 groups = 252 rows.
static_assert(kPackChunkUnits * 12 <= 256 && kPackChunkUnits * 3 <= 64, "chunk exceeds the CRT lift's exact range");
static_assert(kPackRows == kPackUnits * 12 && kPackRows == kPackGroups * 4, "row grouping");

constexpr int kDigitTile = 10;   // mask columns per k_pack_digits workgroup (40 KB of LDS)
static_assert(kn % kDigitTile == 0, "digit tile");

struct PackArgs {
    const uint32_t *key;   // [750][2 primes][2 c][4 rows][4 v][64 L][4 e]   (bk_v2 layout)
    const uint2 *tu_f, *ts_f, *tu_i, *ts_i, *tpost;   // the context's v4 twiddles (blind_rotate_v4.hip V4Args)
    uint32_t qinv_neg0, qinv_neg1, crt_h, crt_hp;
};

// Transpose + decompose + scatter.  Workgroup (x, t): mask columns i0 = 10 x .. i0 + 9 of output t.
// Word (i, j) of dig: (a + kPackOffset) >> 8 for the input placed at j, i.e. the digits d_1 .. d_6
// + 8 in its six nibbles (d_1 highest); 0x888888, the digits of a = 0, where no input is placed.
// pos comes from device memory unchecked by the host: an entry outside [0, kN) drops its input
// before any address is formed from it (the same for every workgroup of the launch).  Duplicate
// positions race on one LDS word or one output word: the output is unspecified, nothing is out of
// bounds.
// The body takes output t's inputs through `in`: in.a(p) the mask of input p from column i0 on,
// in.b(p) its body, in.live(p) false for an input that is dropped (constant true for the strided
// forms); and the position of input p as pos[p], or p * pos_step for a null pos: the kernels below
// differ only in these.
struct PackStrided {   // input p at a fixed stride from input 0
    const int32_t *__restrict__ a0;
    size_t a_p;
    const int32_t *__restrict__ b0;
    size_t b_p;
    __device__ __forceinline__ bool live(int) const { return true; }
    __device__ __forceinline__ const int32_t *a(int p) const { return a0 + (size_t)p * a_p; }
    __device__ __forceinline__ int32_t b(int p) const { return b0[(size_t)p * b_p]; }
};
template <class In>
__device__ __forceinline__ void pack_digits_body(int P, const In in, const int32_t *__restrict__ pos, int pos_step,
                                                 uint32_t *__restrict__ dig, int32_t *__restrict__ out) {
    __shared__ uint32_t tile[kDigitTile][kN];
    uint32_t *flat = &tile[0][0];
    const int tid = threadIdx.x, t = blockIdx.y, i0 = blockIdx.x * kDigitTile;
    for (int k = tid; k < kDigitTile * kN; k += 256) flat[k] = kPackOffset >> 8;
    __syncthreads();
    for (int k = tid; k < P * kDigitTile; k += 256) {
        const int p = k / kDigitTile, c = k - p * kDigitTile;
        const int j = pos ? pos[p] : p * pos_step;
        if (in.live(p) && (unsigned)j < (unsigned)kN) tile[c][j] = ((uint32_t)in.a(p)[c] + kPackOffset) >> 8;
    }
    __syncthreads();
    uint32_t *d = dig + ((size_t)t * kn + i0) * kN;
    for (int k = tid; k < kDigitTile * kN; k += 256) d[k] = flat[k];
    if (blockIdx.x != 0) return;   // uniform: the first workgroup of each output also places b
    __syncthreads();
    for (int k = tid; k < kN; k += 256) tile[0][k] = 0;
    __syncthreads();
    for (int p = tid; p < P; p += 256) {
        const int j = pos ? pos[p] : p * pos_step;
        if (in.live(p) && (unsigned)j < (unsigned)kN) tile[0][j] = (uint32_t)in.b(p);
    }
    __syncthreads();
    int32_t *o = out + (size_t)t * 2 * kN;
    for (int k = tid; k < kN; k += 256) {
        o[k] = 0;
        o[kN + k] = (int32_t)tile[0][k];
    }
}
__global__ __launch_bounds__(256) void k_pack_digits(int P, const int32_t *__restrict__ in_a,
                                                     const int32_t *__restrict__ in_b, const int32_t *__restrict__ pos,
                                                     uint32_t *__restrict__ dig, int32_t *__restrict__ out) {
    const int t = blockIdx.y, i0 = blockIdx.x * kDigitTile;
    pack_digits_body(P, PackStrided{in_a + (size_t)t * P * kn + i0, kn, in_b + (size_t)t * P, 1}, pos, 1, dig, out);
}
// function-major inputs: in_a [P][T_total][kn], in_b [P][T_total], input p of
// output t at coefficient p * pos_step (P * pos_step <= kN is the launcher's check)
__global__ __launch_bounds__(256) void k_pack_digits_fm(int P, int T_total, const int32_t *__restrict__ in_a,
                                                        const int32_t *__restrict__ in_b, int pos_step,
                                                        uint32_t *__restrict__ dig, int32_t *__restrict__ out) {
    const int t = blockIdx.y, i0 = blockIdx.x * kDigitTile;
    pack_digits_body(P, PackStrided{in_a + (size_t)t * kn + i0, (size_t)T_total * kn, in_b + t, (size_t)T_total}, nullptr,
                     pos_step, dig, out);
}
// a circuit level's select rows: output t0 + t = r B + k gathers the p = sel[r].p
// candidates of select row r at instance k from the wire table wa [W][B][kn], wb [W][B], candidate m
// at coefficient m (kN / p).  The record comes from device memory: p is clamped into [0, 16], and a
// wire id outside [0, W) drops that candidate before an address is formed from it (the rule of pos).
struct PackGather {
    const CircSel *__restrict__ rec;
    const int32_t *__restrict__ wa, *__restrict__ wb;
    int W, B, k, i0;
    __device__ __forceinline__ bool live(int p) const { return (unsigned)rec->w[p] < (unsigned)W; }
    __device__ __forceinline__ const int32_t *a(int p) const { return wa + ((size_t)rec->w[p] * B + k) * kn + i0; }
    __device__ __forceinline__ int32_t b(int p) const { return wb[(size_t)rec->w[p] * B + k]; }
};
__global__ __launch_bounds__(256) void k_pack_digits_rows(int B, int W, int t0, const CircSel *__restrict__ sel,
                                                          const int32_t *__restrict__ wa,
                                                          const int32_t *__restrict__ wb, uint32_t *__restrict__ dig,
                                                          int32_t *__restrict__ out) {
    const int t = t0 + blockIdx.y, i0 = blockIdx.x * kDigitTile;
    const int r = t / B, k = t - r * B;
    int P = sel[r].p;
    P = P < 0 ? 0 : P > 16 ? 16 : P;
    pack_digits_body(P, PackGather{sel + r, wa, wb, W, B, k, i0}, nullptr, P ? kN / P : 1, dig, out);
}

// centred CRT lift of lazy residues x0 in [0, 2 q0), x1 in [0, 2 q1), reduced mod 2^32: the lift of
// blind_rotate_v4.hip (crt_lazy), exact for |c| < 2^52
__device__ __forceinline__ uint32_t pack_crt(uint32_t x0, uint32_t x1, uint32_t h, uint32_t hp) {
    const uint32_t d = x1 + 3u * kQ1 - x0;                      // (3 q1 - 2 q0, 5 q1), > 0
    const uint32_t t0 = shoup_lazy(d, h, hp, 0u - kQ1);         // [0, 2 q1)
    const uint32_t t = umin32(t0, t0 - kQ1);                    // [0, q1)
    const uint32_t tc = t > (kQ1 - 1) / 2 ? t - kQ1 : t;
    return x0 + kQ0 * tc;
}

// One key group: S <- S + D (.) K_grp in the NTT domain, S kept Montgomery-reduced.
// D enters as four digit polynomials lifted to [q - 8, q + 7] (< 2q) in layout A.
__device__ __forceinline__ void pack_group(uint32_t (&D)[4][16], uint32_t (&S)[2][16], uint32_t *sc, const PackArgs &g,
                                           int grp, int s, int L, uint32_t q) {
    ntt_fwd<4>(D, sc, g.tu_f + 16 * s, g.ts_f + s * 27 * 64 + L, L, q);   // < 22 q, layout C
    const uint4 *k4 = reinterpret_cast<const uint4 *>(g.key + ((size_t)(grp * 2 + s) * 8) * kN) + L;
    const uint32_t qinv = s ? g.qinv_neg1 : g.qinv_neg0;
    // 2^32 mod q: REDC(S R) = S, so the running sum rides through the group's one reduction
    const uint32_t R = s ? (uint32_t)((1ull << 32) % kQ1) : (uint32_t)((1ull << 32) % kQ0);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            uint4 b[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) b[p] = k4[(c * 4 + p) * 256 + v * 64];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t b0 = e == 0 ? b[0].x : e == 1 ? b[0].y : e == 2 ? b[0].z : b[0].w;
                const uint32_t b1 = e == 0 ? b[1].x : e == 1 ? b[1].y : e == 2 ? b[1].z : b[1].w;
                const uint32_t b2 = e == 0 ? b[2].x : e == 1 ? b[2].y : e == 2 ? b[2].z : b[2].w;
                const uint32_t b3 = e == 0 ? b[3].x : e == 1 ? b[3].y : e == 2 ? b[3].z : b[3].w;
                const int r = 4 * v + e;
                // D < 22 q, key words < q: the four products are < 88 q^2 as in cmux_v4.  The carried
                // term: S < 3.875 q and R < q add < 3.875 q^2, so x < 91.875 q^2 < 2^7 2^54 = 2^61
                // and x + m q < 2^61 + 2^59 fits.  REDC gives < x / 2^32 + q < (91.875 / 32 + 1) q
                // < 3.875 q again (q < 2^27), the invariant of S from S = 0 on.
                const uint64_t x = (uint64_t)D[0][r] * b0 + (uint64_t)D[1][r] * b1 + (uint64_t)D[2][r] * b2 +
                                   (uint64_t)D[3][r] * b3 + (uint64_t)S[c][r] * R;
                const uint32_t m = (uint32_t)x * qinv;
                S[c][r] = (uint32_t)((x + (uint64_t)m * q) >> 32);
            }
        }
    }
}

// Key group 3 u + M of unit u: rows 4 M .. 4 M + 3 of the unit's 12, row = 6 h + (j - 1) for mask
// column 2 u + h and digit j; the digit is nibble 6 - j of the column's word (every index a constant)
template <int M>
__device__ __forceinline__ void pack_unit_group(const uint32_t (&W)[2][16], uint32_t (&S)[2][16], uint32_t *sc,
                                                const PackArgs &g, int u, int s, int L, uint32_t q) {
    uint32_t D[4][16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        constexpr int row0 = 4 * M;
        const int row = row0 + k, h = row / kPackT, sh = 4 * (kPackT - 1 - row % kPackT);
#pragma unroll
        for (int r = 0; r < 16; ++r) D[k][r] = ((W[h][r] >> sh) & 15u) + (q - 8u);
    }
    pack_group(D, S, sc, g, 3 * u + M, s, L, q);
}

// End of a chunk: inverse transform of S, post-twist, exchange of the residues between the two
// waves, lift; wave s keeps the coefficients L + 64 (8 s + rr) of both polynomials in acc.
// ntt_inv_ct documents inputs < 3.75 q; S < 3.875 q still fits: stage 0 gives < 7.875 q (its
// K = 4 q > 3.875 q keeps u + K - v positive), stage 1 < 15.875 q (K = 8 q), the 8 Shoup stages add
// 2 q each: < 31.875 q < 2^32.
__device__ __forceinline__ void pack_flush(uint32_t (&S)[2][16], uint32_t (&acc)[2][8], uint32_t (*scratch)[kPadRow],
                                           const PackArgs &g, int s, int L, uint32_t q) {
    uint32_t *sc = scratch[s];
    ntt_inv_ct<2>(S, sc, g.tu_i + 16 * s, g.ts_i + s * 27 * 64 + L, L, q);
    const uint2 *tp = g.tpost + s * 16 * 64 + L;
    const uint32_t negq = 0u - q;
#pragma unroll
    for (int r = 0; r < 16; ++r) {   // post-twist psi^-n (n = L + 64 r) -> [0, 2q)
        const uint2 w = tp[r * 64];
#pragma unroll
        for (int c = 0; c < 2; ++c) S[c][r] = shoup_lazy(S[c][r], w.x, w.y, negq);
    }
    // wave 0 keeps the registers 0 .. 7 and gives 8 .. 15, wave 1 the other way round (crt4_give / crt4_take)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) sc[(c * 8 + rr) * 64 + L] = s ? S[c][rr] : S[c][8 + rr];
    __syncthreads();
    const uint32_t *other = scratch[1 - s];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            const uint32_t xo = other[(c * 8 + rr) * 64 + L];
            const uint32_t xm = s ? S[c][8 + rr] : S[c][rr];
            acc[c][rr] += pack_crt(s ? xo : xm, s ? xm : xo, g.crt_h, g.crt_hp);
        }
    __syncthreads();   // the other wave has read this wave's scratch before the next transform writes it
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) S[c][r] = 0;
}

// Workgroup (x, t): units [x upw, min((x + 1) upw, 250)) of output t.  Both waves run the same
// trip counts, so every barrier is reached by the whole workgroup.
__global__ __launch_bounds__(kPackThreads, 1) void k_pack_v4(PackArgs g, int upw, int split,
                                                            const uint32_t *__restrict__ dig,
                                                            int32_t *__restrict__ out) {
    __shared__ uint32_t scratch[2][kPadRow];
    const int tid = threadIdx.x;
    const int s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = tid & 63;
    const uint32_t q = s ? kQ1 : kQ0;
    const int t = blockIdx.y;
    const int u0 = blockIdx.x * upw;
    const int u1 = u0 + upw < kPackUnits ? u0 + upw : kPackUnits;
    const uint32_t *dt = dig + (size_t)t * kn * kN + L;
    uint32_t S[2][16], acc[2][8];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int r = 0; r < 16; ++r) S[c][r] = 0;
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) acc[c][rr] = 0;
    }
    int pending = 0;
    for (int u = u0; u < u1; ++u) {
        uint32_t W[2][16];   // the digit words of mask columns 2 u and 2 u + 1, layout A
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r) W[h][r] = dt[(size_t)(2 * u + h) * kN + 64 * r];
        pack_unit_group<0>(W, S, scratch[s], g, u, s, L, q);
        pack_unit_group<1>(W, S, scratch[s], g, u, s, L, q);
        pack_unit_group<2>(W, S, scratch[s], g, u, s, L, q);
        if (++pending == kPackChunkUnits) {
            pack_flush(S, acc, scratch, g, s, L, q);
            pending = 0;
        }
    }
    if (pending) pack_flush(S, acc, scratch, g, s, L, q);
    // OUT -= this slice's sum; coefficient j = L + 64 (8 s + rr) of polynomial c
    uint32_t *o = reinterpret_cast<uint32_t *>(out) + (size_t)t * 2 * kN + L + 64 * 8 * s;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            uint32_t *w = o + c * kN + 64 * rr;
            if (split) atomicAdd(w, 0u - acc[c][rr]);
            else *w -= acc[c][rr];
        }
}

}  // namespace

int pack_split(int T, int cus) {
    if (T <= 0 || cus <= 0) return 1;
    const int G = 2 * cus / T;
    return G < 2 ? 1 : G > kPackUnits / 2 ? kPackUnits / 2 : G;
}

// the gather of launch_pack_rows
struct PackRowsArgs {
    int t0, B, W;
    const CircSel *sel;
};

// fm_total > 0: the function-major form of launch_pack_fm with T_total = fm_total and pos_step;
// rows: the gather form of launch_pack_rows (in_a, in_b the wire table)
static hipError_t pack_launches(const DeviceKey &key, const uint32_t *pack_key, int T, int P, const int32_t *in_a,
                                const int32_t *in_b, const int32_t *pos, int fm_total, int pos_step, uint32_t *dig, int G,
                                int32_t *out, hipStream_t s, const PackRowsArgs *rows = nullptr) {
    if (T <= 0) return hipSuccess;
    if (!pack_key || !key.tw2 || !key.tw4 || T > kPackMaxBatch || P < 1 || P > kN || !in_a || !in_b || !dig || !out ||
        G < 1 || G > kPackUnits)
        return hipErrorInvalidValue;
    if (fm_total > 0 && (T > fm_total || pos_step < 1 || (long)(P - 1) * pos_step >= kN)) return hipErrorInvalidValue;
    PackArgs g;
    g.key = pack_key;
    g.tu_f = key.tw2;
    g.ts_f = key.tw2 + 64;
    g.tu_i = key.tw4;
    g.ts_i = key.tw4 + 32;
    g.tpost = key.tw4 + 32 + 2 * 27 * 64;
    g.qinv_neg0 = key.qinv_neg[0];
    g.qinv_neg1 = key.qinv_neg[1];
    g.crt_h = key.crt_h;
    g.crt_hp = key.crt_hp;
    if (rows) {
        if (!rows->sel || rows->B < 1 || rows->W < 1 || rows->t0 < 0) return hipErrorInvalidValue;
        trace_kernel("k_pack_digits_rows");
        hipLaunchKernelGGL(k_pack_digits_rows, dim3(kn / kDigitTile, T), dim3(256), 0, s, rows->B, rows->W, rows->t0,
                           rows->sel, in_a, in_b, dig, out);
    } else if (fm_total > 0) {
        trace_kernel("k_pack_digits(function-major)");
        hipLaunchKernelGGL(k_pack_digits_fm, dim3(kn / kDigitTile, T), dim3(256), 0, s, P, fm_total, in_a, in_b, pos_step,
                           dig, out);
    } else {
        trace_kernel("k_pack_digits");
        hipLaunchKernelGGL(k_pack_digits, dim3(kn / kDigitTile, T), dim3(256), 0, s, P, in_a, in_b, pos, dig, out);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int upw = (kPackUnits + G - 1) / G;        // units per workgroup
    const int grid = (kPackUnits + upw - 1) / upw;   // no empty slice
    trace_kernel(grid > 1 ? "k_pack_v4(split)" : "k_pack_v4");
    hipLaunchKernelGGL(k_pack_v4, dim3(grid, T), dim3(kPackThreads), 0, s, g, upw, grid > 1 ? 1 : 0, dig, out);
    return hipGetLastError();
}

hipError_t launch_pack(const DeviceKey &key, const uint32_t *pack_key, int T, int P, const int32_t *in_a,
                       const int32_t *in_b, const int32_t *pos, uint32_t *dig, int G, int32_t *out, hipStream_t s) {
    return pack_launches(key, pack_key, T, P, in_a, in_b, pos, 0, 1, dig, G, out, s);
}

hipError_t launch_pack_fm(const DeviceKey &key, const uint32_t *pack_key, int T, int P, int T_total,
                          const int32_t *in_a, const int32_t *in_b, int pos_step, uint32_t *dig, int G, int32_t *out,
                          hipStream_t s) {
    if (T_total <= 0) return hipErrorInvalidValue;
    return pack_launches(key, pack_key, T, P, in_a, in_b, nullptr, T_total, pos_step, dig, G, out, s);
}

hipError_t launch_pack_rows(const DeviceKey &key, const uint32_t *pack_key, int T, int t0, int B, int W,
                            const CircSel *sel, const int32_t *wa, const int32_t *wb, uint32_t *dig, int G,
                            int32_t *out, hipStream_t s) {
    const PackRowsArgs rows{t0, B, W, sel};
    return pack_launches(key, pack_key, T, 16, wa, wb, nullptr, 0, 1, dig, G, out, s, &rows);
}

}  // namespace tfhe_amd
