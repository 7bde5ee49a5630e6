// blind_rotate_v4.hip — v4 blind rotation: v2's register-resident layout with fewer VALU
// instructions per CMux step (the v2 kernel is VALU-issue bound: its time tracks its
// instruction count).
//
// Same contract as v2 (tfhe_blindRotate_FFT + extraction, lwe-bootstrapping-functions-fft.cu
// :676-737, 1408-1456, 1834-1870; tGswFFTExternMulToTLwe tgsw-fft-operations.cu:124-264).
// Changes against v2, all exact (scripts/emu_v4.py checks the index math and the bounds):
//  * inverse transform = Cooley-Tukey DIT on the bit-reversed slots + a psi^-n post-twist
//    (5 VALU per butterfly, no reductions: < 23.75q) instead of Harvey Gentleman-Sande (8);
//  * the MAC's REDC result stays lazy (< 3.75q), the inverse output stays lazy ([0, 2q)) and
//    the CRT lift takes both residues lazily;
//  * the accumulator is kept as a periodic negacyclic extension E[k] = +-acc[k mod N]
//    (k < 3N, sign - when k mod 2N >= N): X^a * ACC at coefficient j is E[(j - a) mod 2N + ...]
//    read with immediate offsets, so the rotation costs no address or sign arithmetic.
#include "br_common.h"
#include "ntt_wave.h"

namespace tfhe_amd {

namespace {

constexpr int kV4Threads = 128;
constexpr int kExt = 3 * kN;

struct V4Shared {
    uint32_t E[2][kExt];               // periodic negacyclic accumulator (a, b), 24 KB
    uint32_t scratch[2][kPadRow];      // one per wave (prime)
    int bara[512];
    int barb;
};

struct V4Args {
    const uint32_t *bk;   // [kn][2][2 c][4 p][4 v][64 L][4 e]   (v2 layout)
    const uint2 *tu_f;    // [2][16] uniform forward twiddles (negated)
    const uint2 *ts_f;    // [2][27][64] forward streams (negated)
    const uint2 *tu_i;    // [2][16] inverse-CT uniform twiddles (negated)
    const uint2 *ts_i;    // [2][27][64] inverse-CT streams (negated)
    const uint2 *tpost;   // [2][16][64] psi^-(L + 64 r), positive
    uint32_t qinv_neg0, qinv_neg1, crt_h, crt_hp;
};

__device__ __forceinline__ void e_store(uint32_t *E, int j, uint32_t v) {
    E[j] = v;
    E[j + kN] = 0u - v;
    E[j + 2 * kN] = v;
}

// centred CRT lift of lazy residues x0 in [0, 2 q0), x1 in [0, 2 q1), reduced mod 2^32.
// The exact external-product coefficient c has |c| < 2^52 << q0 q1 / 2, so the lift
// x0 + q0 tc with tc = (x1 - x0) q0^-1 mod q1 taken in (-q1/2, q1/2] equals c.
__device__ __forceinline__ uint32_t crt_lazy(uint32_t x0, uint32_t x1, uint32_t h, uint32_t hp) {
    const uint32_t d = x1 + 3u * kQ1 - x0;                      // (3 q1 - 2 q0, 5 q1), > 0
    const uint32_t t0 = shoup_lazy(d, h, hp, 0u - kQ1);         // [0, 2 q1)
    const uint32_t t = umin32(t0, t0 - kQ1);                    // [0, q1)
    const uint32_t tc = t > (kQ1 - 1) / 2 ? t - kQ1 : t;
    return x0 + kQ0 * tc;
}

template <int S>
__device__ __forceinline__ void crt4_give(V4Shared &sh, const uint32_t (&O)[2][16], int L) {
    uint32_t *mine = sh.scratch[S];
    constexpr int give = 8 * (1 - S);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) mine[(c * 8 + rr) * 64 + L] = O[c][give + rr];
}
// XP (external product only, tGswFFTExternMulToTLwe): the result replaces the accumulator
template <int S, bool XP = false>
__device__ __forceinline__ void crt4_take(V4Shared &sh, const uint32_t (&O)[2][16], int L, const V4Args &g) {
    const uint32_t *other = sh.scratch[1 - S];
    constexpr int keep = 8 * S;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            const uint32_t xo = other[(c * 8 + rr) * 64 + L];
            const uint32_t xm = O[c][keep + rr];
            const uint32_t x0 = S == 0 ? xm : xo, x1 = S == 0 ? xo : xm;
            const int j = L + 64 * (keep + rr);
            e_store(sh.E[c], j, (XP ? 0u : sh.E[c][j]) + crt_lazy(x0, x1, g.crt_h, g.crt_hp));
        }
}

// one CMux step for key index i and rotation a (1..2N-1); called by both waves.  XP: the
// external product alone, ACC <- BK_i (x) ACC (tgsw-fft-operations.cu:124-264; a unused)
template <bool XP = false>
__device__ __forceinline__ void cmux_v4(V4Shared &sh, const V4Args &g, int i, int a, int s, int L) {
    const uint32_t q = s ? kQ1 : kQ0;
    uint32_t *sc = sh.scratch[s];
    // (X^a - 1) ACC + gadget decomposition (tgsw-functions.cu:300-413), layout A; digits
    // lifted to [q - 512, q + 511]
    uint32_t D[4][16];
    const int base = (L - a) & (k2N - 1);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t t = (XP ? 0u : sh.E[c][base + 64 * r] - sh.E[c][L + 64 * r]) +
                               (XP ? sh.E[c][L + 64 * r] : 0u) + kDecompOffset;
            D[2 * c][r] = ((t >> 22) & 1023u) + (q - 512u);
            D[2 * c + 1][r] = ((t >> 12) & 1023u) + (q - 512u);
        }
    const uint2 *tsf = g.ts_f + s * 27 * 64 + L, *tsi = g.ts_i + s * 27 * 64 + L, *tpb = g.tpost + s * 16 * 64 + L;
    ntt_fwd<4>(D, sc, g.tu_f + 16 * s, tsf, L, q);
    // pointwise MAC with BK_i (layout C: reg r = 4 v + e <-> slot 16 L + r), REDC lazy
    const uint4 *bk4 = reinterpret_cast<const uint4 *>(g.bk + ((size_t)(i * 2 + s) * 8) * kN) + L;
    const uint32_t qinv = s ? g.qinv_neg1 : g.qinv_neg0;
    uint32_t O[2][16];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            uint4 b[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) b[p] = bk4[(c * 4 + p) * 256 + v * 64];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t b0 = e == 0 ? b[0].x : e == 1 ? b[0].y : e == 2 ? b[0].z : b[0].w;
                const uint32_t b1 = e == 0 ? b[1].x : e == 1 ? b[1].y : e == 2 ? b[1].z : b[1].w;
                const uint32_t b2 = e == 0 ? b[2].x : e == 1 ? b[2].y : e == 2 ? b[2].z : b[2].w;
                const uint32_t b3 = e == 0 ? b[3].x : e == 1 ? b[3].y : e == 2 ? b[3].z : b[3].w;
                const int r = 4 * v + e;
                const uint64_t x = (uint64_t)D[0][r] * b0 + (uint64_t)D[1][r] * b1 + (uint64_t)D[2][r] * b2 +
                                   (uint64_t)D[3][r] * b3;                          // < 88 q^2 < 2^61
                const uint32_t m = (uint32_t)x * qinv;
                O[c][r] = (uint32_t)((x + (uint64_t)m * q) >> 32);               // < 3.75 q
            }
        }
    }
    ntt_inv_ct<2>(O, sc, g.tu_i + 16 * s, tsi, L, q);   // < 31.75 q, layout A
    {   // post-twist psi^-n (n = L + 64 r) -> [0, 2q)
        const uint2 *tp = tpb;
        const uint32_t negq = 0u - q;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint2 w = tp[r * 64];
#pragma unroll
            for (int c = 0; c < 2; ++c) O[c][r] = shoup_lazy(O[c][r], w.x, w.y, negq);
        }
    }
    if (s == 0) crt4_give<0>(sh, O, L);
    else crt4_give<1>(sh, O, L);
    __syncthreads();
    if (s == 0) crt4_take<0, XP>(sh, O, L, g);
    else crt4_take<1, XP>(sh, O, L, g);
    __syncthreads();
}

// prologue + modswitch + 500 CMux steps + extraction of one ciphertext into (ua, *ub).
// LUT (programmable bootstrap, compile-time): the accumulator starts from the test vector tv [kN]
// in device memory; tv = null (a constant row beside LUT rows) keeps the constant (mu, ..., mu)
// MANY (many-LUT bootstrap; implies LUT): the modulus switch to a multiple of
// 2^mo.th and the extraction of the coefficients 0 .. mo.n_out - 1 (modarith.h ManyOut)
// TLWE (bootstrap from an encrypted accumulator; excludes LUT and MANY): the
// accumulator starts from X^{2N - barb} (acc_a, acc_b), the TLWE sample at acc_src [2][kN]
template <bool LUT = false, bool MANY = false, bool TLWE = false>
__device__ __forceinline__ void br_v4_body(V4Shared &sh, const V4Args &g, const RowTerms &t, int32_t mu,
                                           int32_t *__restrict__ ua, int32_t *__restrict__ ub,
                                           const int32_t *__restrict__ tv = nullptr,
                                           const ManyOut &mo = ManyOut{},
                                           const int32_t *__restrict__ acc_src = nullptr) {
    const int tid = threadIdx.x;
    const int s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = tid & 63;
    br_prologue<MANY, kV4Threads>(t, mo.th, tid, sh.bara, sh.barb);
    __syncthreads();
    if constexpr (TLWE) {   // both rows of the periodic extension from the sample (modarith.h lut_coeff)
        const int e = (k2N - sh.barb) & (k2N - 1);
        for (int k = tid; k < kExt; k += kV4Threads) {
            sh.E[0][k] = lut_coeff(acc_src, k, e);
            sh.E[1][k] = lut_coeff(acc_src + kN, k, e);
        }
    } else if (LUT && tv) {   // ACC = (0, X^{2N - barb} tv) as its periodic extension (modarith.h lut_coeff)
        const int e = (k2N - sh.barb) & (k2N - 1);
        for (int k = tid; k < kExt; k += kV4Threads) {
            sh.E[0][k] = 0;
            sh.E[1][k] = lut_coeff(tv, k, e);
        }
    } else {   // ACC = (0, X^{2N - barb} (mu, ..., mu)) (:1427-1431), as its periodic extension
        const int e = (k2N - sh.barb) & (k2N - 1);
        for (int k = tid; k < kExt; k += kV4Threads) {
            sh.E[0][k] = 0;
            sh.E[1][k] = ((k - e) & (k2N - 1)) < kN ? (uint32_t)mu : 0u - (uint32_t)mu;
        }
    }
    __syncthreads();
    for (int i = 0; i < kn; ++i) {
        const int a = sh.bara[i];
        if (a == 0) continue;            // X^0 - 1 = 0: identity CMux (:705)
        cmux_v4(sh, g, i, a, s, L);
    }
    // sample extraction at index 0 (lwe.cu:41-56): a_j = -acc_a[N - j] = E_a[2N - j]
    for (int j = tid; j < kN; j += kV4Threads) ua[j] = (int32_t)sh.E[0][(k2N - j) & (k2N - 1)];
    if (tid == 0) *ub = (int32_t)sh.E[1][0];
    if constexpr (MANY) {   // extraction at index f: a_j = E_a[(f - j) mod 2N], b = acc_b[f]
        for (int f = 1; f < mo.n_out; ++f) {
            int32_t *uf = mo.ua1 + (size_t)(f - 1) * mo.stride * kN;
            for (int j = tid; j < kN; j += kV4Threads) uf[j] = (int32_t)sh.E[0][(f - j) & (k2N - 1)];
        }
        if (tid >= 1 && tid < mo.n_out) mo.ub1[(size_t)(tid - 1) * mo.stride] = (int32_t)sh.E[1][tid];
    }
}

// Guard mode (engine.h Guard): the fp64 kernel ran first and flagged each ciphertext with its
// largest rounding distance; a ciphertext under the threshold keeps its result (the workgroup
// exits before touching anything), one at or above it is recomputed here exactly.
struct V4Guard {
    const uint32_t *flags;   // null: not in guard mode
    uint32_t hi;             // threshold (high word of the distance)
    uint32_t *stats;         // [0]: recomputed ciphertexts
};
__device__ __forceinline__ bool guard_skip(const V4Guard &gd, size_t slot) {
    if (!gd.flags) return false;
    const uint32_t f0 = gd.flags[2 * slot], f1 = gd.flags[2 * slot + 1];
    if ((f0 > f1 ? f0 : f1) < gd.hi) return true;   // uniform over the workgroup
    if (threadIdx.x == 0) atomicAdd(gd.stats, 1u);
    return false;
}

// gate batch: ciphertext gct of half h = gct / B reads in_h at index gct mod B.  Grid-stride
// over the total ciphertexts: one per workgroup normally; in guard mode a small grid scans the
// flags (almost always all clear) instead of dispatching one workgroup per ciphertext.
// MINW: waves per SIMD the register budget is cut for — 2 for the exact throughput kernel
// (tfhe_amd_select_kernel(4): 256 VGPRs, 27 spilled), 1 for the guard launch (284 VGPRs, no scratch: a
// kernel with a private segment costs ~12 us more per dispatch even when every workgroup exits
// at once)
template <int MINW, bool LUT = false, bool MANY = false, bool TLWE = false>
__global__ __launch_bounds__(kV4Threads, MINW) void k_blind_rotate_v4(V4Args g, int B, int total, BrInput in0,
                                                                BrInput in1, int32_t mu,
                                                                int32_t *__restrict__ u_a,
                                                                int32_t *__restrict__ u_b, V4Guard gd) {
    __shared__ V4Shared sh;
    bool used = false;
    for (int gct = blockIdx.x; gct < total; gct += gridDim.x) {
        if (guard_skip(gd, (size_t)gct)) continue;
        if (used) __syncthreads();   // the previous ciphertext's extraction has read the LDS
        used = true;
        const int half = gct >= B;
        const int idx = half ? gct - B : gct;
        const BrInput &in = half ? in1 : in0;
        RowTerms t;
        row_terms<LUT>(t, in, idx);
        const LutArgs l = lut_args<LUT, MANY>(in, B, idx, gct, u_a, u_b);
        br_v4_body<LUT, MANY, TLWE>(sh, g, t, mu, u_a + (size_t)gct * kN, u_b + gct, l.tv, l.mo,
                                    acc_sample<TLWE>(in, idx));
    }
}

// circuit level: flat slot r B + k (row r, instance k < B), grid-stride as the gate kernel;
// wires are [W][B] ciphertexts, the extracted sample of (r, k) goes to u slot r B + k
// TLWE (a level's select rows): slot r B + k starts from the TLWE sample of the same
// index in acc, formed here from the slot alone
template <int MINW, bool LUT = false, bool MANY = false, bool TLWE = false>
__global__ __launch_bounds__(kV4Threads, MINW) void k_blind_rotate_v4_rows(V4Args g, int B, long total,
                                                                     const CircRow *__restrict__ rows,
                                                                     const int32_t *__restrict__ wa,
                                                                     const int32_t *__restrict__ wb, int32_t mu,
                                                                     int32_t *__restrict__ u_a,
                                                                     int32_t *__restrict__ u_b, V4Guard gd,
                                                                     const int32_t *__restrict__ acc) {
    static_assert(!TLWE || (!LUT && !MANY), "the tlwe form excludes the table forms");
    __shared__ V4Shared sh;
    bool used = false;
    for (long slot = blockIdx.x; slot < total; slot += gridDim.x) {
        if (guard_skip(gd, (size_t)slot)) continue;
        if (used) __syncthreads();
        used = true;
        const int r = (int)(slot / B), k = (int)(slot - (long)r * B);
        const CircRow row = rows[r];
        RowTerms t;
        row_terms(t, row, wa, wb, B, k);
        const LutArgs l = lut_args<LUT, MANY>(rows + r, row, B, k, u_a, u_b);
        br_v4_body<LUT, MANY, TLWE>(sh, g, t, mu, u_a + (size_t)slot * kN, u_b + slot, l.tv, l.mo,
                                    TLWE ? acc + (size_t)slot * 2 * kN : nullptr);
    }
}

// Mixed-key rows: slot = row r of one instance, grid-stride as above; each row is
// computed (guard mode: recomputed when its flag says so) under the key of its own slot
// (br_common.h ring_key) and reads its inputs in place from the caller's arrays (engine.h RingWires).
template <int MINW, bool LUT = false>
__global__ __launch_bounds__(kV4Threads, MINW) void k_blind_rotate_v4_rows_mk(V4Args g, RingKeys kr, long total,
                                                                        const CircRow *__restrict__ rows,
                                                                        RingWires wr, RingLut lt, int32_t mu,
                                                                        int32_t *__restrict__ u_a,
                                                                        int32_t *__restrict__ u_b, V4Guard gd) {
    __shared__ V4Shared sh;
    bool used = false;
    for (long slot = blockIdx.x; slot < total; slot += gridDim.x) {
        if (guard_skip(gd, (size_t)slot)) continue;
        if (used) __syncthreads();
        used = true;
        const CircRow row = rows[slot];
        RowTerms t;
        row_terms(t, row, wr);
        V4Args gk = g;
        gk.bk = ring_key<uint32_t>(kr, slot);
        const int32_t *tv = nullptr;
        if constexpr (LUT) tv = lut_table(lt.tv, lt.lut_index, lt.n_lut, ring_entry(row.x, wr.n));
        br_v4_body<LUT, false, false>(sh, gk, t, mu, u_a + (size_t)slot * kN, u_b + slot, tv);
    }
}

// Mixed-key circuit levels: k_blind_rotate_v4_rows with the key of the instance's own
// slot (br_common.h ring_inst_key); flat slot r B + k, guard flags of the same index.  Modes Const, Lut
// and Many.
template <int MINW, bool LUT = false, bool MANY = false>
__global__ __launch_bounds__(kV4Threads, MINW) void k_blind_rotate_v4_rows_mkc(V4Args g, RingInstKeys kr, int B,
                                                                         long total, const CircRow *__restrict__ rows,
                                                                         const int32_t *__restrict__ wa,
                                                                         const int32_t *__restrict__ wb, int32_t mu,
                                                                         int32_t *__restrict__ u_a,
                                                                         int32_t *__restrict__ u_b, V4Guard gd) {
    __shared__ V4Shared sh;
    bool used = false;
    for (long slot = blockIdx.x; slot < total; slot += gridDim.x) {
        if (guard_skip(gd, (size_t)slot)) continue;
        if (used) __syncthreads();
        used = true;
        const int r = (int)(slot / B), k = (int)(slot - (long)r * B);
        const CircRow row = rows[r];
        RowTerms t;
        row_terms(t, row, wa, wb, B, k);
        V4Args gk = g;
        gk.bk = ring_inst_key<uint32_t>(kr, k);
        const LutArgs l = lut_args<LUT, MANY>(rows + r, row, B, k, u_a, u_b);
        br_v4_body<LUT, MANY, false>(sh, gk, t, mu, u_a + (size_t)slot * kN, u_b + slot, l.tv, l.mo);
    }
}

__global__ __launch_bounds__(kV4Threads, 2) void k_blind_rotate_v4_debug(V4Args g, int iters, int32_t *__restrict__ acc,
                                                                      const int32_t *__restrict__ bara) {
    __shared__ V4Shared sh;
    const int tid = threadIdx.x;
    const int s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = tid & 63;
    int32_t *accg = acc + (size_t)blockIdx.x * 2 * kN;
    for (int j = tid; j < 2 * kN; j += kV4Threads) e_store(sh.E[j >> kLogN], j & (kN - 1), (uint32_t)accg[j]);
    for (int i = tid; i < iters; i += kV4Threads) sh.bara[i] = bara[(size_t)blockIdx.x * iters + i] & (k2N - 1);
    __syncthreads();
    for (int i = 0; i < iters; ++i) {
        const int a = sh.bara[i];
        if (a == 0) continue;
        cmux_v4(sh, g, i, a, s, L);
    }
    for (int j = tid; j < 2 * kN; j += kV4Threads) accg[j] = (int32_t)sh.E[j >> kLogN][j & (kN - 1)];
}

// tGswFFTExternMulToTLwe batch: accumulator b (acc [B][2][kN]) <- BK_{key_index[b]} (x) acc, exact
__global__ __launch_bounds__(kV4Threads, 2) void k_external_product_v4(V4Args g, const int32_t *__restrict__ key_index,
                                                                        int32_t *__restrict__ acc) {
    __shared__ V4Shared sh;
    const int tid = threadIdx.x;
    const int s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = tid & 63;
    int32_t *accg = acc + (size_t)blockIdx.x * 2 * kN;
    // the index comes from device memory unchecked by the host: outside [0, kn) the accumulator is
    // left as it is (whole workgroup, uniform) rather than reading past the key
    const int i = key_index[blockIdx.x];
    if (i < 0 || i >= kn) return;
    for (int j = tid; j < 2 * kN; j += kV4Threads) e_store(sh.E[j >> kLogN], j & (kN - 1), (uint32_t)accg[j]);
    __syncthreads();
    cmux_v4<true>(sh, g, i, 0, s, L);
    for (int j = tid; j < 2 * kN; j += kV4Threads) accg[j] = (int32_t)sh.E[j >> kLogN][j & (kN - 1)];
}

// ---- leveled mode on caller-supplied TGSW samples: g.bk points at an imported
// set (engine.h TgswLookup / TgswCmux), everything else in g is the context's.

// A selector index read from device memory, the same word for the whole workgroup.
__device__ __forceinline__ int tgsw_sel(const int32_t *p) { return __builtin_amdgcn_readfirstlane(*p); }

// Table lookup: one workgroup per query q.  ACC = table t (trivial sample (0, tab) for tab_rows = 1),
// then d_h CMux steps on the query's selectors: step i rotates by X^{-2^(i + log_stride)} when the
// selector encrypts 1, so that coefficient f of the result is tab[(addr << log_stride) + f]; the
// extraction is the many-LUT epilogue's (br_v4_body), output f of query q to u sample f B + q.
// A selector outside [0, count) skips its step (uniform) and never forms an address.
__global__ __launch_bounds__(kV4Threads, 2) void k_tgsw_lookup_v4(V4Args g, TgswLookup a,
                                                                   int32_t *__restrict__ u_a,
                                                                   int32_t *__restrict__ u_b) {
    __shared__ V4Shared sh;
    const int tid = threadIdx.x;
    const int s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = tid & 63;
    const int q = blockIdx.x;
    const int32_t *src;
    int rows = a.tab_rows;
    if (a.per_query) {   // the CMux tree's result, one sample per query
        src = a.tab + (size_t)q * 2 * kN;
        rows = 2;
    } else {
        int t = a.tab_index ? tgsw_sel(a.tab_index + q) : 0;
        t = t < 0 ? 0 : t >= a.n_tab ? a.n_tab - 1 : t;   // clamped before any address is formed
        src = a.tab + (size_t)t * a.tab_stride;
    }
    for (int j = tid; j < kN; j += kV4Threads) {
        e_store(sh.E[0], j, rows == 2 ? (uint32_t)src[j] : 0u);
        e_store(sh.E[1], j, (uint32_t)src[(rows - 1) * kN + j]);
    }
    __syncthreads();
    for (int i = 0; i < a.d_h; ++i) {
        const int idx = tgsw_sel(a.sel + (size_t)q * a.sel_stride + i);
        if (idx < 0 || idx >= a.count) continue;
        cmux_v4(sh, g, idx, k2N - (1 << (i + a.log_stride)), s, L);
    }
    for (int f = 0; f < a.n_out; ++f) {   // extraction at index f: a_j = E_a[(f - j) mod 2N], b = acc_b[f]
        int32_t *uf = u_a + ((size_t)f * a.B + q) * kN;
        for (int j = tid; j < kN; j += kV4Threads) uf[j] = (int32_t)sh.E[0][(f - j) & (k2N - 1)];
    }
    if (tid < a.n_out) u_b[(size_t)tid * a.B + q] = (int32_t)sh.E[1][tid];
}

// CMux batch: out[w] = d0[w] + C_{sel} (x) (d1[w] - d0[w]), the XP path of cmux_v4 on the difference.
// Pair w belongs to query w / ppq.  n_poly > 0: the pair's operands are the polynomials 2 j, 2 j + 1
// (j = w mod ppq) of the query's table, read in place; else d0 / d1 + w pair_stride (d0 null: the
// plain external product).  Each workgroup reads its operands whole before it writes, so out may be
// d0 or d1.  A selector outside [0, count) gives out = d0.
__global__ __launch_bounds__(kV4Threads, 2) void k_tgsw_cmux_v4(V4Args g, TgswCmux a) {
    __shared__ V4Shared sh;
    const int tid = threadIdx.x;
    const int s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = tid & 63;
    const int w = blockIdx.x;
    const int q = w / a.ppq;
    const int32_t *d0, *d1;
    int rows = 2;
    if (a.n_poly > 0) {
        int t = a.tab_index ? tgsw_sel(a.tab_index + q) : 0;
        t = t < 0 ? 0 : t >= a.n_tab ? a.n_tab - 1 : t;
        rows = a.rows;
        d0 = a.d0 + ((size_t)t * a.n_poly + 2 * (w - q * a.ppq)) * rows * kN;
        d1 = d0 + (size_t)rows * kN;
    } else {
        d0 = a.d0 ? a.d0 + (size_t)w * a.pair_stride : nullptr;
        d1 = a.d1 + (size_t)w * a.pair_stride;
    }
    const int idx = tgsw_sel(a.sel + (size_t)q * a.sel_stride);
    const bool live = idx >= 0 && idx < a.count;
    // word j of an operand, j < 2 kN; rows = 1: the mask is zero and the body is the one row
    auto word = [&](const int32_t *d, int j) -> uint32_t {
        if (!d || (rows == 1 && j < kN)) return 0u;
        return (uint32_t)d[rows == 1 ? j - kN : j];
    };
    for (int j = tid; j < 2 * kN; j += kV4Threads)
        e_store(sh.E[j >> kLogN], j & (kN - 1), word(d1, j) - word(d0, j));
    __syncthreads();   // d1 is in the LDS: out may overwrite it
    if (live) cmux_v4<true>(sh, g, idx, 0, s, L);
    // d0 is read again word by word, each by the thread that then writes that word: out may be d0
    int32_t *out = a.out + (size_t)w * 2 * kN;
    for (int j = tid; j < 2 * kN; j += kV4Threads)
        out[j] = (int32_t)(word(d0, j) + (live ? sh.E[j >> kLogN][j & (kN - 1)] : 0u));
}

// Leveled automaton, one step over one input bit (engine.h TgswDfaStep): workgroup w
// computes state st = live[w mod n_live] of query q = w / n_live,
//   out = d0 + C_sel (x) (d1 - d0 + 2^11 on every word), d_b = the sample of state next[st][b],
// the XP path of cmux_v4 on the difference.  The 2^11 centres the decomposition's truncation (it
// drops 12 bits of every word): the product reads only the digits, so nothing else changes.  The
// operands come from the source buffer, the result goes to the destination buffer at the state's own
// slot, and the two buffers are distinct: within a launch no workgroup reads what another writes.
// FIRST: the operands are the final weights (rows = 1: the mask is zero).  LAST: the result (the
// start state's) is extracted as in k_tgsw_lookup_v4 instead of being stored.
// Every index read from device memory is wave-uniform and checked before an address is formed: a
// state or transition outside [0, Q) ends the workgroup, a selector outside [0, count) and a state
// with next0 == next1 (whose product is exactly zero) give out = d0, fin_index is clamped.
// TW (transition weights): d_b gains w_b = w_val[st][b] at coefficient p = *w_pos of
// its b polynomial, so the thread that owns word kN + p adds w1 - w0 to the difference and w0 to the
// result; the state copies only when w0 == w1 too.  A p outside [0, kN) makes the step weightless.
template <bool FIRST, bool LAST, bool TW>
__global__ __launch_bounds__(kV4Threads, 2) void k_tgsw_dfa_v4(V4Args g, TgswDfaStep a) {
    __shared__ V4Shared sh;
    const int tid = threadIdx.x;
    const int s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = tid & 63;
    const int w = blockIdx.x;
    const int q = w / a.n_live;
    if (q >= a.B) return;
    const int st = tgsw_sel(a.live + (w - q * a.n_live));
    if (st < 0 || st >= a.Q) return;
    const int n0 = tgsw_sel(a.next + 2 * st), n1 = tgsw_sel(a.next + 2 * st + 1);
    if (n0 < 0 || n0 >= a.Q || n1 < 0 || n1 >= a.Q) return;
    int rows = 2;
    const int32_t *base;
    if constexpr (FIRST) {
        int t = a.fin_index ? tgsw_sel(a.fin_index + q) : 0;
        t = t < 0 ? 0 : t >= a.n_fin ? a.n_fin - 1 : t;
        rows = a.fin_rows;
        base = a.fin + (size_t)t * a.Q * rows * kN;
    } else {
        base = a.src + (size_t)q * a.Q * 2 * kN;
    }
    const int32_t *d0 = base + (size_t)n0 * rows * kN, *d1 = base + (size_t)n1 * rows * kN;
    const int idx = tgsw_sel(a.sel + (size_t)q * a.sel_stride);
    uint32_t w0 = 0u, w1 = 0u;
    int wj = -1;   // the word of the weighted coefficient, j = kN + p; -1: a weightless step
    if constexpr (TW) {
        const int p = tgsw_sel(a.w_pos);
        if (p >= 0 && p < kN) {
            wj = kN + p;
            w0 = (uint32_t)tgsw_sel(a.w_val + 2 * st);
            w1 = (uint32_t)tgsw_sel(a.w_val + 2 * st + 1);
        }
    }
    const bool live = (n0 != n1 || w0 != w1) && idx >= 0 && idx < a.count;
    // word j of an operand, j < 2 kN; rows = 1: the mask is zero and the body is the one row
    auto word = [&](const int32_t *d, int j) -> uint32_t {
        if (rows == 1 && j < kN) return 0u;
        return (uint32_t)d[rows == 1 ? j - kN : j];
    };
    // what the transition weight adds to word j: w on the one word kN + p, nothing elsewhere
    auto weight = [&](int j, uint32_t w) -> uint32_t { return TW && j == wj ? w : 0u; };
    if (live) {
        for (int j = tid; j < 2 * kN; j += kV4Threads)
            e_store(sh.E[j >> kLogN], j & (kN - 1), word(d1, j) - word(d0, j) + (1u << 11) + weight(j, w1 - w0));
        __syncthreads();
        cmux_v4<true>(sh, g, idx, 0, s, L);
    }
    if constexpr (!LAST) {
        int32_t *out = a.dst + ((size_t)q * a.Q + st) * 2 * kN;
        for (int j = tid; j < 2 * kN; j += kV4Threads)
            out[j] = (int32_t)(word(d0, j) + weight(j, w0) + (live ? sh.E[j >> kLogN][j & (kN - 1)] : 0u));
    } else {
        // each thread replaces the words it read: the sum as the periodic extension the extraction reads
        for (int j = tid; j < 2 * kN; j += kV4Threads) {
            uint32_t *E = sh.E[j >> kLogN];
            const int k = j & (kN - 1);
            e_store(E, k, word(d0, j) + weight(j, w0) + (live ? E[k] : 0u));
        }
        __syncthreads();
        for (int f = 0; f < a.n_out; ++f) {   // extraction at index f: a_j = E_a[(f - j) mod 2N], b = acc_b[f]
            int32_t *uf = a.u_a + ((size_t)f * a.u_stride + q) * kN;
            for (int j = tid; j < kN; j += kV4Threads) uf[j] = (int32_t)sh.E[0][(f - j) & (k2N - 1)];
        }
        if (tid < a.n_out) a.u_b[(size_t)tid * a.u_stride + q] = (int32_t)sh.E[1][tid];
    }
}

unsigned brv10(unsigned x) {
    unsigned r = 0;
    for (int i = 0; i < kLogN; i++) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
}

}  // namespace

// Inverse-CT and post-twist tables of the v4 kernel, host side, consumption order.
// psi^-m for m < N is ipsi[brv(m)] (ntt_tables.h).
void build_v4_twiddles(const NttTables &t, uint2 *tu_i, uint2 *ts_i, uint2 *tpost) {
    for (int s = 0; s < 2; ++s) {
        const uint32_t q = kQ[s];
        auto ipow = [&](unsigned m) { return t.ipsi[s][brv10(m)]; };
        auto shp = [&](uint32_t w) { return (uint32_t)(((uint64_t)w << 32) / q); };
        auto neg = [&](uint32_t w) { return make_uint2(0u - w, shp(w)); };
        tu_i[s * 16 + 15] = make_uint2(0, 0);
        for (int S = 0; S <= 3; ++S)
            for (int p = 0; p < (1 << S); ++p) tu_i[s * 16 + (1 << S) - 1 + p] = neg(ipow((unsigned)p << (10 - S)));
        int slot = 0;
        for (int S = 4; S <= 9; ++S) {
            const int cnt = S <= 5 ? 1 << (S - 2) : 1 << (S - 6);
            for (int g = 0; g < cnt; ++g, ++slot)
                for (int L = 0; L < 64; ++L) {
                    const unsigned p = S <= 5 ? (unsigned)((L & 3) | (g << 2)) : (unsigned)(L + 64 * g);
                    ts_i[(s * 27 + slot) * 64 + L] = neg(ipow(p << (10 - S)));
                }
        }
        for (int r = 0; r < 16; ++r)
            for (int L = 0; L < 64; ++L) {
                const uint32_t w = ipow((unsigned)(L + 64 * r));
                tpost[(s * 16 + r) * 64 + L] = make_uint2(w, shp(w));
            }
    }
}

static V4Args v4_args(const DeviceKey &key) {
    V4Args g;
    g.bk = key.bk_v2;
    g.tu_f = key.tw2;
    g.ts_f = key.tw2 + 64;
    g.tu_i = key.tw4;
    g.ts_i = key.tw4 + 32;
    g.tpost = key.tw4 + 32 + 2 * 27 * 64;
    g.qinv_neg0 = key.qinv_neg[0];
    g.qinv_neg1 = key.qinv_neg[1];
    g.crt_h = key.crt_h;
    g.crt_hp = key.crt_hp;
    return g;
}

constexpr int kGuardGrid = 256;
static V4Guard v4_guard(const Guard *guard) {
    V4Guard gd{nullptr, 0u, nullptr};
    if (guard && guard->flags) gd = V4Guard{guard->flags, guard_threshold_hi(), guard->stats};
    return gd;
}

// MINW (the kernels' first template argument): 1 for the guard launch, 2 for the exact one
hipError_t launch_blind_rotate_v4(const DeviceKey &key, int B, int halves, const BrInput *in, int32_t mu,
                                  int32_t *u_a, int32_t *u_b, hipStream_t s, const Guard *guard) {
    if (B <= 0) return hipSuccess;
    if (!key.bk_v2) return hipErrorInvalidValue;
    BrMode mode;   // the guard launch recomputes a flagged ciphertext from the same table
    if (br_mode(in, halves, &mode) != hipSuccess) return hipErrorInvalidValue;
    const BrInput in1 = halves > 1 ? in[1] : in[0];
    const V4Guard gd = v4_guard(guard);
    const int total = B * halves;
    // guard mode: 256 workgroups scan the flags (B = 1024: 15 -> ~4 us per launch)
    const int grid = gd.flags && total > kGuardGrid ? kGuardGrid : total;
    trace_kernel(KernelLabel("k_blind_rotate_v4", mode, {gd.flags ? "guard" : nullptr}).s);
    with_mode(mode, [&](auto m) {
        with_flag(gd.flags != nullptr, [&](auto f) {
            hipLaunchKernelGGL((k_blind_rotate_v4<decltype(f)::value ? 1 : 2, mode_lut(decltype(m)::value),
                                                  mode_many(decltype(m)::value), mode_tlwe(decltype(m)::value)>),
                               dim3(grid), dim3(kV4Threads), 0, s, v4_args(key), B, total, in[0], in1, mu, u_a, u_b, gd);
        });
    });
    return hipGetLastError();
}

hipError_t launch_blind_rotate_v4_rows(const DeviceKey &key, int B, int nrows, const CircRow *rows, const int32_t *wa,
                                       const int32_t *wb, int32_t mu, int32_t *u_a, int32_t *u_b, hipStream_t s,
                                       BrMode mode, const Guard *guard) {
    if (B <= 0 || nrows <= 0) return hipSuccess;
    if (!key.bk_v2 || mode == BrMode::Tlwe) return hipErrorInvalidValue;   // the tlwe rows form has its own launcher
    const V4Guard gd = v4_guard(guard);
    const long total = (long)B * nrows;
    const long grid = gd.flags && total > kGuardGrid ? kGuardGrid : total < 0x7fffffffL ? total : 0x7fffffffL;
    trace_kernel(KernelLabel("k_blind_rotate_v4_rows", mode, {gd.flags ? "guard" : nullptr}).s);
    with_mode(mode, [&](auto m) {
        with_flag(gd.flags != nullptr, [&](auto f) {
            hipLaunchKernelGGL((k_blind_rotate_v4_rows<decltype(f)::value ? 1 : 2, mode_lut(decltype(m)::value),
                                                       mode_many(decltype(m)::value)>),
                               dim3((unsigned)grid), dim3(kV4Threads), 0, s, v4_args(key), B, total, rows, wa, wb, mu, u_a,
                               u_b, gd, (const int32_t *)nullptr);
        });
    });
    return hipGetLastError();
}

hipError_t launch_blind_rotate_v4_rows_ring(const DeviceKey &key, const RingKeys &keys, int nrows, const CircRow *rows,
                                            const RingWires &wires, const RingLut &lut, int32_t mu, int32_t *u_a,
                                            int32_t *u_b, hipStream_t s, BrMode mode, const Guard *guard) {
    if (nrows <= 0) return hipSuccess;
    if (!key.tw2 || !key.tw4 || !keys.bk || !keys.row_key || keys.n_keys < 1 || !rows || wires.n < 1)
        return hipErrorInvalidValue;
    if (mode != BrMode::Const && mode != BrMode::Lut) return hipErrorInvalidValue;
    if (mode == BrMode::Lut && (!lut.tv || lut.n_lut < 1)) return hipErrorInvalidValue;
    const V4Guard gd = v4_guard(guard);
    const long total = nrows;
    const long grid = gd.flags && total > kGuardGrid ? kGuardGrid : total;
    trace_kernel(KernelLabel("k_blind_rotate_v4_rows", mode, {"multi-key", gd.flags ? "guard" : nullptr}).s);
    with_flag(mode == BrMode::Lut, [&](auto m) {
        with_flag(gd.flags != nullptr, [&](auto f) {
            hipLaunchKernelGGL((k_blind_rotate_v4_rows_mk<decltype(f)::value ? 1 : 2, decltype(m)::value>),
                               dim3((unsigned)grid), dim3(kV4Threads), 0, s, v4_args(key), keys, total, rows, wires, lut,
                               mu, u_a, u_b, gd);
        });
    });
    return hipGetLastError();
}

hipError_t launch_blind_rotate_v4_rows_ringc(const DeviceKey &key, const RingInstKeys &keys, int B, int nrows,
                                             const CircRow *rows, const int32_t *wa, const int32_t *wb, int32_t mu,
                                             int32_t *u_a, int32_t *u_b, hipStream_t s, BrMode mode, const Guard *guard) {
    if (B <= 0 || nrows <= 0) return hipSuccess;
    if (!key.tw2 || !key.tw4 || !keys.bk || !keys.inst_key || keys.n_keys < 1 || !rows || mode == BrMode::Tlwe)
        return hipErrorInvalidValue;
    const V4Guard gd = v4_guard(guard);
    const long total = (long)B * nrows;
    const long grid = gd.flags && total > kGuardGrid ? kGuardGrid : total < 0x7fffffffL ? total : 0x7fffffffL;
    trace_kernel(KernelLabel("k_blind_rotate_v4_rows", mode, {"multi-key", "circuit", gd.flags ? "guard" : nullptr}).s);
    with_mode(mode, [&](auto m) {
        with_flag(gd.flags != nullptr, [&](auto f) {
            if constexpr (!mode_tlwe(decltype(m)::value))
                hipLaunchKernelGGL((k_blind_rotate_v4_rows_mkc<decltype(f)::value ? 1 : 2, mode_lut(decltype(m)::value),
                                                               mode_many(decltype(m)::value)>),
                                   dim3((unsigned)grid), dim3(kV4Threads), 0, s, v4_args(key), keys, B, total, rows, wa, wb,
                                   mu, u_a, u_b, gd);
        });
    });
    return hipGetLastError();
}

hipError_t launch_blind_rotate_v4_rows_tlwe(const DeviceKey &key, int B, int nrows, const CircRow *rows,
                                            const int32_t *wa, const int32_t *wb, const int32_t *acc, int32_t *u_a,
                                            int32_t *u_b, hipStream_t s, const Guard *guard) {
    if (B <= 0 || nrows <= 0) return hipSuccess;
    if (!key.bk_v2 || !acc || !rows) return hipErrorInvalidValue;
    const V4Guard gd = v4_guard(guard);
    const long total = (long)B * nrows;
    const long grid = gd.flags && total > kGuardGrid ? kGuardGrid : total < 0x7fffffffL ? total : 0x7fffffffL;
    trace_kernel(KernelLabel("k_blind_rotate_v4_rows", BrMode::Tlwe, {gd.flags ? "guard" : nullptr}).s);
    with_flag(gd.flags != nullptr, [&](auto f) {
        hipLaunchKernelGGL((k_blind_rotate_v4_rows<decltype(f)::value ? 1 : 2, false, false, true>), dim3((unsigned)grid),
                           dim3(kV4Threads), 0, s, v4_args(key), B, total, rows, wa, wb, (int32_t)0, u_a, u_b, gd, acc);
    });
    return hipGetLastError();
}

hipError_t launch_external_product_v4(const DeviceKey &key, int B, const int32_t *key_index, int32_t *acc,
                                      hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (!key.bk_v2) return hipErrorInvalidValue;
    trace_kernel("k_external_product_v4");
    hipLaunchKernelGGL(k_external_product_v4, dim3(B), dim3(kV4Threads), 0, s, v4_args(key), key_index, acc);
    return hipGetLastError();
}

// the context's twiddles and CRT constants with an imported set in the key's place
static bool tgsw_args(const DeviceKey &key, const uint32_t *set, int count, V4Args *g) {
    if (!set || count <= 0 || !key.tw2 || !key.tw4) return false;
    *g = v4_args(key);
    g->bk = set;
    return true;
}

hipError_t launch_tgsw_lookup_v4(const DeviceKey &key, const uint32_t *set, const TgswLookup &a, int32_t *u_a,
                                 int32_t *u_b, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    V4Args g;
    if (!tgsw_args(key, set, a.count, &g) || !a.tab || !u_a || !u_b || (a.d_h > 0 && !a.sel) || a.d_h < 0 ||
        a.log_stride < 0 || a.d_h + a.log_stride > kLogN || a.n_out < 1 || a.n_out > 16 ||
        a.n_out > (1 << a.log_stride) || (!a.per_query && (a.n_tab < 1 || a.tab_rows < 1 || a.tab_rows > 2)))
        return hipErrorInvalidValue;
    trace_kernel("k_tgsw_lookup_v4");
    hipLaunchKernelGGL(k_tgsw_lookup_v4, dim3(a.B), dim3(kV4Threads), 0, s, g, a, u_a, u_b);
    return hipGetLastError();
}

hipError_t launch_tgsw_cmux_v4(const DeviceKey &key, const uint32_t *set, int pairs, const TgswCmux &a,
                               hipStream_t s, const char *label) {
    if (pairs <= 0) return hipSuccess;
    V4Args g;
    if (!tgsw_args(key, set, a.count, &g) || !a.sel || (!a.d1 && a.n_poly <= 0) || !a.out || a.ppq < 1 ||
        (a.n_poly > 0 && (!a.d0 || a.n_tab < 1 || a.rows < 1 || a.rows > 2 || a.ppq * 2 != a.n_poly)))
        return hipErrorInvalidValue;
    trace_kernel(label ? label : "k_tgsw_cmux_v4");
    hipLaunchKernelGGL(k_tgsw_cmux_v4, dim3(pairs), dim3(kV4Threads), 0, s, g, a);
    return hipGetLastError();
}

hipError_t launch_tgsw_dfa_v4(const DeviceKey &key, const uint32_t *set, const TgswDfaStep &a, bool first, bool last,
                              hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    V4Args g;
    if (!tgsw_args(key, set, a.count, &g) || !a.sel || !a.next || !a.live || a.Q < 1 || a.Q > 64 || a.n_live < 1 ||
        a.n_live > a.Q || (long)a.B * a.n_live > 0x7fffffffL)
        return hipErrorInvalidValue;
    if (first ? (!a.fin || a.n_fin < 1 || a.fin_rows < 1 || a.fin_rows > 2) : !a.src) return hipErrorInvalidValue;
    const bool tw = a.w_val != nullptr;   // transition weights: both arrays or neither
    if (tw != (a.w_pos != nullptr)) return hipErrorInvalidValue;
    if (last ? (a.n_live != 1 || !a.u_a || !a.u_b || a.n_out < 1 || a.n_out > (tw ? 64 : 16) || a.u_stride < a.B)
             : (!a.dst || a.dst == a.src))
        return hipErrorInvalidValue;
    if (tw)
        trace_kernel(first ? (last ? "k_tgsw_dfa_v4(weights+tw+extract)" : "k_tgsw_dfa_v4(weights+tw)")
                           : (last ? "k_tgsw_dfa_v4(tw+extract)" : "k_tgsw_dfa_v4(tw)"));
    else
        trace_kernel(first ? (last ? "k_tgsw_dfa_v4(weights+extract)" : "k_tgsw_dfa_v4(weights)")
                           : (last ? "k_tgsw_dfa_v4(extract)" : "k_tgsw_dfa_v4"));
    with_flag(first, [&](auto fi) {
        with_flag(last, [&](auto la) {
            with_flag(tw, [&](auto we) {
                hipLaunchKernelGGL((k_tgsw_dfa_v4<decltype(fi)::value, decltype(la)::value, decltype(we)::value>),
                                   dim3(a.B * a.n_live), dim3(kV4Threads), 0, s, g, a);
            });
        });
    });
    return hipGetLastError();
}

hipError_t launch_blind_rotate_v4_debug(const DeviceKey &key, int B, int iters, int32_t *acc, const int32_t *bara,
                                        hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (iters < 0 || iters > kn) return hipErrorInvalidValue;
    trace_kernel("k_blind_rotate_v4_debug");
    hipLaunchKernelGGL(k_blind_rotate_v4_debug, dim3(B), dim3(kV4Threads), 0, s, v4_args(key), iters, acc, bara);
    return hipGetLastError();
}

}  // namespace tfhe_amd
