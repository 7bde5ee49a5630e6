// engine.h — internal device-engine interface (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "params.h"
#include "ntt_tables.h"

namespace tfhe_amd {

// Key material of one cloud key resident on one GPU.
struct DeviceKey {
    int device = -1;
    uint32_t *bk_ntt = nullptr;   // upload only (freed once repacked): [kn][2 primes][kKpl][2][kN], Montgomery form, 1/N folded
    uint32_t *bk_v2 = nullptr;    // the exact (v4) kernels' key: [kn][2 primes][2 c][kKpl][4 v][64 L][4 e] (same values)
    uint2 *tw2 = nullptr;         // v4 forward twiddles: uniform fwd/inv [2][16] x2, streams [2][27][64], [2][18][64]
    uint2 *tw4 = nullptr;         // v4 inverse-CT twiddles: uniform [2][16], streams [2][27][64], post-twist [2][16][64]
    double2 *bk_fft = nullptr;    // v6: [kn][4 rows][2 c][8 r][64 L] FFT-domain key / 512 (slot 8 L + r)
    double2 *tw6 = nullptr;       // v6 twiddles: forward [4] + [4][64] x 2, inverse [4][64] x 2, post-twist [8][64]
    int32_t *ksk = nullptr;       // [kN][kKsT][3][kKsRow]   (digits h = 1..3)
    int32_t *ksk4 = nullptr;      // ks-v4: [126 column blocks][kN][kKsT][3][4]
    int32_t *ksk5 = nullptr;      // ks-v5 (int8 MFMA): [64 N-blocks][kN][64 lanes][16 B] signed key bytes
    NttTables *tables = nullptr;  // device copy
    uint32_t qinv_neg[2] = {0, 0};
    uint32_t crt_h = 0, crt_hp = 0;
    bool has_bk = false;
};
constexpr int kTw2Words = 2 * 16 * 2 + 2 * 27 * 64 + 2 * 18 * 64;   // uint2 entries
constexpr int kTw4Words = 2 * 16 + 2 * 27 * 64 + 2 * 16 * 64;
// double2 entries (blind_rotate_v6.hip build_v6_twiddles)
constexpr int kTw6Words = 4 + 4 * 4 * 64 + 8 * 64 + 2 * 64;   // fft_wave.h table map

// x = (0, c) + sa * X + sb * Y   (gate prologue, boot-gates.cu:98-397; Y unused if sb == 0)
// Programmable bootstrap: with tv set the accumulator starts from the caller's
// test vector, ACC = (0, X^{2N - barb} tv[t]), instead of the constant (mu, ..., mu), and the
// launchers pick the kernels' LUT instantiation.  tv = [n_lut][kN] on the device; ciphertext g
// takes table t = lut_index[g] (null: table 0), clamped by the kernel into [0, n_lut) before any
// address is formed.  The launchers' mu is unused then.
// Many-LUT bootstrap: n_out >= 1 picks the kernels' many-LUT instantiation (one
// half only).  The prologue switches to a multiple of nu = 2^log_nu and the epilogue extracts the
// coefficients f = 0 .. n_out - 1 of the rotated accumulator; output f of ciphertext g goes to u
// sample f B + g, so u holds n_out B samples.  n_out = 0: the single-table launch above.
// With tv set the input may have a third term: x = (0, c) + sa * X + sb * Y + sc * Z.
// Which of the three forms a launch takes is its BrMode (br_mode below), derived once per launch.
struct BrInput {
    const int32_t *x_a, *x_b;
    const int32_t *y_a, *y_b;
    int32_t c, sa, sb;
    int32_t n_lut = 0;
    const int32_t *tv = nullptr;
    const int32_t *lut_index = nullptr;
    int32_t log_nu = 0, n_out = 0;
    // third input: x += sc * Z.  Only the LUT and many-LUT instantiations read
    // it (sc != 0 needs tv and z_a, z_b); the constant kernels keep two inputs.
    const int32_t *z_a = nullptr, *z_b = nullptr;
    int32_t sc = 0;
    // bootstrap from an encrypted accumulator: with acc set the accumulator starts
    // from X^{2N - barb} (acc_a, acc_b), a TLWE sample out of acc [n_acc][2][kN] (a, then b) on the
    // device, instead of a trivial sample.  Ciphertext g takes sample acc_index[g], clamped by the
    // kernel into [0, n_acc) before any address is formed; a null index means sample 0 when
    // n_acc == 1 and sample g otherwise.  One half, two input terms, no tables, one output; the
    // guard launch recomputes a flagged ciphertext from the same sample, so u must not alias acc.
    const int32_t *acc = nullptr;
    const int32_t *acc_index = nullptr;
    int32_t n_acc = 0;
};

// One bootstrapped row of a circuit level (circuit.cpp): the blind rotation input is
// (0, c) + sa W[x] + sb W[y] + sc W[z] over wire indices (-1 = absent; x is always present).
// lut: 0 = the constant test vector (mu, ..., mu); otherwise the row's test vector of kN words
// starts `lut` 32-bit words after the row's own record, in the same device allocation (the level
// tables and the circuit's LUT tables are uploaded as one block, so the offset is the same on every
// device).  Only launches of mode Lut or Many read it.
// many (launches of mode Many): 0 = one output; otherwise log_nu | n_out << 8 of a
// many-LUT row.  Output 0 of row r goes to u row r like every row's; outputs
// f >= 1 go to the u rows urow + f - 1, which lie behind the level's nrows rows.
struct CircRow {
    int32_t c, sa, sb, sc;
    int32_t x, y, z, lut;
    int32_t many = 0, urow = 0;
};
// One key-switched circuit output: W[out] = KS(u[r1] (+ u[r2] if r2 >= 0) + (0, add_b)).
struct CircKs {
    int32_t r1, r2, add_b, out;
};
// One bootstrap-free node: W[out] = (0, c) + s W[in]   (in = -1: the trivial sample (0, c)).
struct CircLin {
    int32_t c, s, in, out;
};

// One select row of a circuit level: the p candidate wires whose samples the digit
// pass of the pack gathers, candidate m to coefficient m kN / p.  The row's selector is a CircRow of
// its own.  The pack's digit kernel reads the record from device memory: p is clamped into [0, 16]
// and a wire id outside [0, W) drops that candidate before an address is formed.
struct CircSel {
    int32_t p;
    int32_t w[16];
};

// Makes `device` current for the scope of an entry point and gives the caller's current device
// back at its end: a caller that works on another GPU (torch.cuda.set_device(1), then a
// context on device 0) keeps its own current device, which HIP and torch allocate on.
struct DeviceScope {
    int prev = -1;
    hipError_t rc;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        rc = device >= 0 && device != prev ? hipSetDevice(device) : hipSuccess;
    }
    ~DeviceScope() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

// Orders the reuse of a scratch buffer across streams.  Device-API callers may pass a different
// stream per call; a call on another stream than the previous user's waits (on the device) for
// the event recorded after that user's last launch, so two batches in flight never share the
// extracted samples u_a / u_b.
struct StreamFence {
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;   // compared only; the event carries the ordering
    hipError_t acquire(hipStream_t s) const {
        return ev && last != s ? hipStreamWaitEvent(s, ev, 0) : hipSuccess;
    }
    hipError_t done(hipStream_t s) {
        if (!ev) {
            const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        last = s;
        return hipEventRecord(ev, s);
    }
    void release() {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
        last = nullptr;
    }
};

// Exactness guard of the fp64 FFT blind rotation.  The v6 kernel rounds each
// external-product coefficient c to the nearest integer; that equals the exact product while the
// FFT error stays below 1/2.  Every wave tracks the largest rounding distance |c - rint(c)| it
// sees over all 500 steps and stores its high word (monotone in the distance) in flags[2 slot + w];
// an exact-NTT (v4) launch in guard mode then recomputes every ciphertext whose flag reaches the
// threshold (1/8 by default) and exits at once for all others.  stats[0] counts the recomputed
// ciphertexts, stats[1] holds the largest high word seen (tfhe_amd_guard_stats).
struct Guard {
    uint32_t *flags = nullptr;
    uint32_t *stats = nullptr;
};
uint32_t guard_threshold_hi();

// The form of a blind-rotation launch, i.e. which instantiation of the kernels it takes: the
// constant test vector (mu, ..., mu), caller-supplied test vectors (programmable bootstrap), or
// test vectors with several extracted outputs (many-LUT; implies Lut).  A rows launch is told its
// mode (the row records are in device memory): Lut if some row of the level carries a test vector
// (CircRow.lut), Many if some row is a many-LUT row (CircRow.many).
// Tlwe: the accumulator starts from an encrypted TLWE sample (BrInput.acc); gate launches, and the
// rows launches of a circuit level's select rows (launch_blind_rotate_*_rows_tlwe below).
enum class BrMode { Const, Lut, Many, Tlwe };
// The mode of a launch over in[0 .. halves), or hipErrorInvalidValue for an inconsistent one.
inline hipError_t br_mode(const BrInput *in, int halves, BrMode *mode) {
    const BrInput &in1 = halves > 1 ? in[1] : in[0];
    // encrypted accumulator: one half, at least one sample, and none of the table forms' fields
    if (in[0].acc || in1.acc) {
        if (halves != 1 || in[0].n_acc <= 0 || in[0].tv || in[0].n_out != 0 || in[0].sc) return hipErrorInvalidValue;
        *mode = BrMode::Tlwe;
        return hipSuccess;
    }
    // programmable bootstrap: every half carries its tables (n_lut >= 1), or none does
    const bool lut = in[0].tv != nullptr;
    if (lut != (in1.tv != nullptr) || (lut && (in[0].n_lut <= 0 || in1.n_lut <= 0))) return hipErrorInvalidValue;
    // many-LUT: one half, tables, log_nu in [0, 4], n_out in [1, 2^log_nu]
    const bool many = in[0].n_out != 0;
    if (many && (!lut || halves != 1 || in[0].log_nu < 0 || in[0].log_nu > 4 || in[0].n_out < 1 ||
                 in[0].n_out > (1 << in[0].log_nu)))
        return hipErrorInvalidValue;
    // third input: only the LUT instantiations read it
    for (const BrInput *h : {&in[0], &in1})
        if (h->sc && (!lut || !h->z_a || !h->z_b)) return hipErrorInvalidValue;
    *mode = many ? BrMode::Many : lut ? BrMode::Lut : BrMode::Const;
    return hipSuccess;
}

// BK conversion (coefficient -> NTT domain) on the device; d_bk_coef = [kn][4][2][kN]
hipError_t launch_bk_to_ntt(const int32_t *d_bk_coef, uint32_t *d_bk_ntt, const NttTables *d_tab,
                            hipStream_t s);
// the NTT-domain key layouts and their twiddle streams (ntt_key.hip), used by the v4 kernels
void build_v2_twiddles(const NttTables &t, uint2 *tu_f, uint2 *tu_i, uint2 *ts_f, uint2 *ts_i);
hipError_t launch_bk_v1_to_v2(const uint32_t *d_v1, uint32_t *d_v2, hipStream_t s);
// v4 (v2 layout, inverse CT + lazy CRT + periodic accumulator), blind_rotate_v4.hip
void build_v4_twiddles(const NttTables &t, uint2 *tu_i, uint2 *ts_i, uint2 *tpost);
// Blind rotation + sample extraction for `halves` x B ciphertexts (v4 and v6 alike): ciphertext g
// of half h reads in[h] at index g and writes u[h*B + g] (u_a row stride kN).
// guard != null: guard mode (recompute only the ciphertexts whose v6 flag reached the threshold)
hipError_t launch_blind_rotate_v4(const DeviceKey &key, int B, int halves, const BrInput *in, int32_t mu,
                                  int32_t *u_a, int32_t *u_b, hipStream_t s, const Guard *guard = nullptr);
hipError_t launch_blind_rotate_v4_debug(const DeviceKey &key, int B, int iters, int32_t *acc,
                                        const int32_t *bara, hipStream_t s);
// tGswFFTExternMulToTLwe, exact (v4 arithmetic): acc [B][2][kN] <- BK_{key_index[b]} (x) acc
hipError_t launch_external_product_v4(const DeviceKey &key, int B, const int32_t *key_index, int32_t *acc,
                                      hipStream_t s);
// ---- leveled mode on caller-supplied TGSW samples (tgsw.cpp).  `set` is `count`
// samples in the bk_v2 layout; twiddles and CRT constants are the key's (KS-only contexts have them).
// Table lookup, one workgroup per query q < B: ACC = table t = tab_index[q] (null: 0; clamped into
// [0, n_tab)) at tab + t tab_stride, tab_rows = 1 a plaintext polynomial (mask 0), 2 a TLWE sample
// (a, b); per_query: ACC = the sample tab + q 2 kN instead (the CMux tree's result).  Then d_h CMux
// steps with the selectors sel[q sel_stride + i] and rotations 2N - 2^(i + log_stride), and the
// extraction of the coefficients f < n_out into u sample f B + q.
struct TgswLookup {
    int B = 0, count = 0;
    const int32_t *sel = nullptr;
    int sel_stride = 0, d_h = 0, log_stride = 0, n_out = 1;
    const int32_t *tab = nullptr;
    long tab_stride = 0;
    int n_tab = 1, tab_rows = 1, per_query = 0;
    const int32_t *tab_index = nullptr;
};
// CMux batch, one workgroup per pair w: out[w] = d0 + C_sel (x) (d1 - d0), out [pairs][2][kN];
// the selector of pair w is sel[(w / ppq) sel_stride].  n_poly > 0 (the first tree level): d0 is the
// table [n_tab][n_poly][rows][kN], pair w takes the polynomials 2 j, 2 j + 1 (j = w mod ppq, ppq =
// n_poly / 2) of table tab_index[w / ppq]; n_poly = 0: operands at d0 / d1 + w pair_stride (d0 null:
// the plain external product of d1).
struct TgswCmux {
    int count = 0;
    const int32_t *sel = nullptr;
    int sel_stride = 1, ppq = 1;
    const int32_t *d0 = nullptr, *d1 = nullptr;
    long pair_stride = 2 * kN;
    int n_poly = 0, rows = 2, n_tab = 1;
    const int32_t *tab_index = nullptr;
    int32_t *out = nullptr;
};
hipError_t launch_tgsw_lookup_v4(const DeviceKey &key, const uint32_t *set, const TgswLookup &a, int32_t *u_a,
                                 int32_t *u_b, hipStream_t s);
// label: the name the launch trace gets (null: "k_tgsw_cmux_v4")
hipError_t launch_tgsw_cmux_v4(const DeviceKey &key, const uint32_t *set, int pairs, const TgswCmux &a,
                               hipStream_t s, const char *label = nullptr);
// One step of a leveled automaton (tgsw_dfa.cpp), one workgroup per (query q < B,
// live state): for every s = live[k], k < n_live,
//   dst[q][s] = d0 + C_sel[q sel_stride] (x) (d1 - d0 + 2^11 on every word), d_b = src[q][next[s][b]],
// over state buffers [B][Q][2][kN] indexed by state id; src and dst are distinct buffers.  A state
// with next[s][0] == next[s][1] and a selector outside [0, count) give dst = d0.
// first: the operands are the final weights fin [n_fin][Q][fin_rows][kN] of table fin_index[q] (null:
// 0; clamped into [0, n_fin)) instead of src; fin_rows = 1: the trivial sample (0, fin).
// last: the result is not stored but extracted at the coefficients f < n_out into u sample
// f u_stride + q (the lookup kernel's index rule); n_live is 1 then (the start state).
struct TgswDfaStep {
    int B = 0, count = 0, Q = 0;
    const int32_t *sel = nullptr;
    int sel_stride = 1;
    const int32_t *next = nullptr;   // [Q][2]
    const int32_t *live = nullptr;
    int n_live = 0;
    const int32_t *src = nullptr;
    int32_t *dst = nullptr;
    const int32_t *fin = nullptr;
    int n_fin = 1, fin_rows = 1;
    const int32_t *fin_index = nullptr;
    int n_out = 1;
    long u_stride = 0;
    int32_t *u_a = nullptr, *u_b = nullptr;
    // transition weights, both or neither: w_val [Q][2] Torus32, w_pos the one
    // word of this step's coefficient position p.  d_b gains w_val[s][b] X^p on its b polynomial, a
    // state copies only when its two weights are equal too, a p outside [0, kN) makes the step
    // weightless; n_out may be up to 64 then.
    const int32_t *w_val = nullptr, *w_pos = nullptr;
};
hipError_t launch_tgsw_dfa_v4(const DeviceKey &key, const uint32_t *set, const TgswDfaStep &a, bool first, bool last,
                              hipStream_t s);
// count-taking forms of launch_bk_to_ntt / launch_bk_v1_to_v2 (the same kernels over `count` samples)
hipError_t launch_tgsw_to_ntt(const int32_t *d_coef, uint32_t *d_ntt, const NttTables *d_tab, int count,
                              hipStream_t s);
hipError_t launch_tgsw_v1_to_v2(const uint32_t *d_v1, uint32_t *d_v2, int count, hipStream_t s);
// ---- LWE -> TLWE packing key switch (pack.cpp, pack_v4.hip).  pack_key: the 750 row
// groups in the bk_v2 layout; dig: scratch of T * kn * kN words.  T <= kPackMaxBatch outputs of P
// inputs each, in_a [T][P][kn], in_b [T][P], pos [P] (null: pos[p] = p), out [T][2][kN].  Two
// launches, k_pack_digits and k_pack_v4; G > 1 splits the key rows of each output over G workgroups
// ("k_pack_v4(split)").  pack_split: the G the entry points use for T outputs on `cus` compute units.
int pack_split(int T, int cus);
hipError_t launch_pack(const DeviceKey &key, const uint32_t *pack_key, int T, int P, const int32_t *in_a,
                       const int32_t *in_b, const int32_t *pos, uint32_t *dig, int G, int32_t *out, hipStream_t s);
// The pack of p-way selection: as launch_pack with function-major inputs, in_a
// [P][T_total][kn] and in_b [P][T_total] offset to the first of the T outputs of this launch, and
// input p at coefficient p * pos_step.  The digit kernel's trace name is "k_pack_digits(function-major)".
hipError_t launch_pack_fm(const DeviceKey &key, const uint32_t *pack_key, int T, int P, int T_total,
                          const int32_t *in_a, const int32_t *in_b, int pos_step, uint32_t *dig, int G, int32_t *out,
                          hipStream_t s);
// The pack of a circuit level's select rows: as launch_pack for the outputs
// t0 .. t0 + T - 1 of the level, output t = r B + k gathering the candidates of select row r (sel[r])
// at instance k from the wire table wa [W][B][kn], wb [W][B]; out is offset to output t0.  The digit
// kernel's trace name is "k_pack_digits_rows".
hipError_t launch_pack_rows(const DeviceKey &key, const uint32_t *pack_key, int T, int t0, int B, int W,
                            const CircSel *sel, const int32_t *wa, const int32_t *wb, uint32_t *dig, int G,
                            int32_t *out, hipStream_t s);
// Box fill (tlwe_box_fill.hip): out = in * (1 + X + ... + X^(2^log_w - 1)), negacyclic, exact mod 2^32,
// over the 2 T polynomials of T TLWE samples [T][2][kN]; out may be in
hipError_t launch_tlwe_box_fill(int T, int log_w, const int32_t *in, int32_t *out, hipStream_t s);
// circuit level (v4 kernel): B instances x nrows rows, wires [W][B] ciphertexts, u slots r B + k
hipError_t launch_blind_rotate_v4_rows(const DeviceKey &key, int B, int nrows, const CircRow *rows, const int32_t *wa,
                                       const int32_t *wb, int32_t mu, int32_t *u_a, int32_t *u_b, hipStream_t s,
                                       BrMode mode, const Guard *guard = nullptr);
// v6 (fp64 FFT external product, the reference's arithmetic), blind_rotate_v6.hip
void build_v6_twiddles(double2 *tw);
hipError_t launch_bk_to_fft(const int32_t *d_bk_coef, double2 *d_bkf, const double2 *d_tw, hipStream_t s);
// guard != null: write the rounding-distance flags (Guard) for the guard launch that follows
hipError_t launch_blind_rotate_v6(const DeviceKey &key, int B, int halves, const BrInput *in, int32_t mu,
                                  int32_t *u_a, int32_t *u_b, hipStream_t s, const Guard *guard = nullptr);
hipError_t launch_blind_rotate_v6_rows(const DeviceKey &key, int B, int nrows, const CircRow *rows, const int32_t *wa,
                                       const int32_t *wb, int32_t mu, int32_t *u_a, int32_t *u_b, hipStream_t s,
                                       BrMode mode, const Guard *guard = nullptr);
hipError_t launch_blind_rotate_v6_debug(const DeviceKey &key, int B, int iters, int32_t *acc,
                                        const int32_t *bara, hipStream_t s);
// The rows launches of a level's select rows, mode Tlwe: row r at instance k starts
// from sample r B + k of acc [nrows B][2][kN] (the index is formed on the device from r, B, k alone)
// and rotates it by the row's selector; u slot and guard flags r B + k as in the other rows launches.
// u must not alias acc (the guard launch recomputes a flagged slot from the same sample).
hipError_t launch_blind_rotate_v6_rows_tlwe(const DeviceKey &key, int B, int nrows, const CircRow *rows,
                                            const int32_t *wa, const int32_t *wb, const int32_t *acc, int32_t *u_a,
                                            int32_t *u_b, hipStream_t s, const Guard *guard = nullptr);
hipError_t launch_blind_rotate_v4_rows_tlwe(const DeviceKey &key, int B, int nrows, const CircRow *rows,
                                            const int32_t *wa, const int32_t *wb, const int32_t *acc, int32_t *u_a,
                                            int32_t *u_b, hipStream_t s, const Guard *guard = nullptr);
// which blind-rotation kernel runs: 0 = default (v6), 4 = exact NTT (tfhe_amd_select_kernel)
int br_version();
// Launch trace: every launcher names the kernel (and variant) it enqueues; a batch entry point of
// the C ABI collects the names of its launches into its context (tfhe_amd_last_kernels), so a
// smoke or bench run can say which kernels produced the results it checked.
void trace_kernel(const char *name);
// circuit level blind rotation with the selected kernel (the rows variant of v6 or v4); the default
// fp64 kernel runs guarded (flags: 2 words per row x instance), the exact one does not use the guard
hipError_t launch_blind_rotate_rows(const DeviceKey &key, int B, int nrows, const CircRow *rows, const int32_t *wa,
                                    const int32_t *wb, int32_t mu, int32_t *u_a, int32_t *u_b, hipStream_t s,
                                    BrMode mode, const Guard *guard);
// the same for a level's select rows (circuit_select.cpp): mode Tlwe from the samples
// acc [nrows B][2][kN], v6 then the guard launch of v4, or v4 alone under tfhe_amd_select_kernel(4)
hipError_t launch_blind_rotate_rows_tlwe(const DeviceKey &key, int B, int nrows, const CircRow *rows, const int32_t *wa,
                                         const int32_t *wb, const int32_t *acc, int32_t *u_a, int32_t *u_b,
                                         hipStream_t s, const Guard *guard);

// ---- mixed-key rows (keyring.cpp): one rows launch over ciphertexts of several cloud
// keys.  Row r runs under key slot row_key[r], clamped by the kernel into [0, n_keys) before the slot's
// key pointer is loaded from bk (bk_fft pointers for the v6 launch, bk_v2 pointers for the v4 one);
// twiddles and CRT constants come from the DeviceKey the launcher is given.  One instance per row.
struct RingKeys {
    const void *const *bk;     // [n_keys] device table of per-slot key pointers
    const int32_t *row_key;    // [nrows] device
    int32_t n_keys;
};
// The rows' inputs stay in the caller's arrays: wire w of a ring row is entry w >> 2 (clamped into
// [0, n)) of input array w & 3 (a0 / a1 / a2; 3 and a null array: absent), -1 absent as in CircRow.
struct RingWires {
    const int32_t *a0, *b0, *a1, *b1, *a2, *b2;
    int32_t n;
};
// mode Lut: the row whose x wire is entry i takes table lut_index[i] (null: 0; clamped) of tv [n_lut][kN]
struct RingLut {
    const int32_t *tv = nullptr;
    const int32_t *lut_index = nullptr;
    int32_t n_lut = 0;
};
// The geometry, rotation and priority policy of launch_blind_rotate_v6_rows (modes Const and Lut);
// trace name "k_blind_rotate_v6_rows(multi-key+...)".
hipError_t launch_blind_rotate_v6_rows_ring(const DeviceKey &key, const RingKeys &keys, int nrows, const CircRow *rows,
                                            const RingWires &wires, const RingLut &lut, int32_t mu, int32_t *u_a,
                                            int32_t *u_b, hipStream_t s, BrMode mode, const Guard *guard = nullptr);
// the exact kernel over the same rows, in guard mode (guard set) or alone
hipError_t launch_blind_rotate_v4_rows_ring(const DeviceKey &key, const RingKeys &keys, int nrows, const CircRow *rows,
                                            const RingWires &wires, const RingLut &lut, int32_t mu, int32_t *u_a,
                                            int32_t *u_b, hipStream_t s, BrMode mode, const Guard *guard = nullptr);
// bootstrap-free ring entries: res[e.out] = (0, e.c) + e.s W[e.in] over ring wires (in = -1: trivial)
hipError_t launch_ring_linear(int nlin, const CircLin *lin, const RingWires &wires, int32_t *res_a, int32_t *res_b,
                              hipStream_t s);

// ---- mixed-key circuit levels (keyring_circuit.cpp): the rows launch of a circuit
// level over B instances of several cloud keys.  Flat slot r B + k, wires [W][B] and the row records
// as in launch_blind_rotate_*_rows (modes Const, Lut and Many); instance k runs under key slot
// inst_key[k], clamped by the kernel into [0, n_keys) before the slot's key pointer is loaded from bk.
struct RingInstKeys {
    const void *const *bk;      // [n_keys] device table of per-slot key pointers (bk_fft / bk_v2)
    const int32_t *inst_key;    // [B] device
    int32_t n_keys;
};
// geometry, rotation and priority policy of launch_blind_rotate_v6_rows; trace name
// "k_blind_rotate_v6_rows(<mode>+multi-key+circuit+<rotation>)"
hipError_t launch_blind_rotate_v6_rows_ringc(const DeviceKey &key, const RingInstKeys &keys, int B, int nrows,
                                             const CircRow *rows, const int32_t *wa, const int32_t *wb, int32_t mu,
                                             int32_t *u_a, int32_t *u_b, hipStream_t s, BrMode mode,
                                             const Guard *guard = nullptr);
// the exact kernel over the same slots, in guard mode (guard set) or alone; trace name
// "k_blind_rotate_v4_rows(<mode>+multi-key+circuit[+guard])"
hipError_t launch_blind_rotate_v4_rows_ringc(const DeviceKey &key, const RingInstKeys &keys, int B, int nrows,
                                             const CircRow *rows, const int32_t *wa, const int32_t *wb, int32_t mu,
                                             int32_t *u_a, int32_t *u_b, hipStream_t s, BrMode mode,
                                             const Guard *guard = nullptr);
// The key switch of such a level in one launch over all key groups (k_keyswitch_v5 with the tiled
// lane map).  The instances are sorted by slot: group g holds the instances order[offsets[g] ..
// offsets[g + 1]), and its lanes, nks offsets[g] + o n_g + j for output o and the group's j-th
// instance, are cut into M-tiles of ks5_tile_lanes() lanes that never span two groups.  Tile t runs
// under the ksk5 of tiles[t].slot (clamped into [0, n_keys) before the slot's table entry is loaded),
// starts at lane tiles[t].first and has tiles[t].live lanes; the padding lanes are never stored.
// The per-slot table names each member's ksk5 by its distance from base5 in 16-byte units (device
// allocations are 256-byte aligned): the kernel adds it to the kernel argument base5, so the key
// stream's loads keep a kernel-argument base like the single-key launches' (a pointer loaded from a
// table cost the kernel 48 bytes of scratch a lane).
struct KsTile {
    int32_t slot, first, live;
};
struct RingKsTiles {
    const void *base5;          // the ksk5 of some member (slot 0's)
    const int64_t *ksk5_off;    // [n_keys] device: (slot's ksk5 - base5) / 16
    const int32_t *order;       // [B] device
    const int32_t *offsets;     // [n_keys + 1] device
    const KsTile *tiles;        // [ntiles] device
    int32_t n_keys, ntiles;
};
int ks5_tile_lanes();
// trace name "k_keyswitch_v5(int8-mfma+multi-key[+splitN])"
hipError_t launch_keyswitch_rows_tiles(const RingKsTiles &t, int B, int nks, const CircKs *ks, const int32_t *u_a,
                                       const int32_t *u_b, int32_t *wa, int32_t *wb, hipStream_t s);
// the key switch of one key group of such a level through the single-key kernels: nks outputs x the n
// instances inst[0 .. n) (device; clamped into [0, B)) of a wire table of stride B; lane t = o n + j
hipError_t launch_keyswitch_rows_inst(const DeviceKey &key, int B, int nks, const CircKs *ks, const int32_t *inst,
                                      int n, const int32_t *u_a, const int32_t *u_b, int32_t *wa, int32_t *wb,
                                      hipStream_t s);

// which key-switch kernel the larger batches take: 5 (int8 MFMA), or 4 with TFHE_AMD_KS5=0
int ks_version();
size_t ksk_v4_words();
size_t ksk_v5_words();
bool ks5_enabled();   // env TFHE_AMD_KS5=0: ks-v4 instead of the int8 MFMA key switch
hipError_t launch_ksk_to_v5(const int32_t *d_ksk, int32_t *d_ksk5, hipStream_t s);
// circuit level key switch: nks outputs x B instances; lane t = g B + k
hipError_t launch_keyswitch_rows(const DeviceKey &key, int B, int nks, const CircKs *ks, const int32_t *u_a,
                                 const int32_t *u_b, int32_t *wa, int32_t *wb, hipStream_t s);
// bootstrap-free nodes: nlin x B instances
hipError_t launch_circuit_linear(int B, int nlin, const CircLin *lin, int32_t *wa, int32_t *wb, hipStream_t s);
hipError_t launch_ksk_to_v4(const int32_t *d_ksk, int32_t *d_ksk4, hipStream_t s);
// current_variance of B key-switched samples u (halves = 2: u1 + u2) from the key-switching key's
// row variances var [kN][kKsT][kKsBase] (reference order of the double adds), into out [B]
hipError_t launch_ks_variance(const int32_t *u_a, int B, int halves, const double *var, double *out, hipStream_t s);
hipError_t launch_ks_variance_rows(const int32_t *u_a, int B, const CircKs *ks, const double *var, double *out,
                                   hipStream_t s);
// Key switch of u (+ u2 if non-null) + (0, add_b) -> res (n=500).
hipError_t launch_keyswitch(const DeviceKey &key, int B, const int32_t *u_a, const int32_t *u_b,
                            const int32_t *u2_a, const int32_t *u2_b, int32_t add_b,
                            int32_t *res_a, int32_t *res_b, hipStream_t s);

// What an entry point outside engine.cpp (tgsw.cpp) sees of a context while it holds it.
struct ContextFrame {
    const DeviceKey *key;
    int device;
    hipStream_t stream;       // the caller's stream, or the context's own
    int32_t *u_a, *u_b;       // the extracted-sample scratch, at least u_slots samples (null if none asked)
};

}  // namespace tfhe_amd

// Runs fn inside the frame every device entry point of engine.cpp sets up: context lock, its device
// current, launch trace open; with u_slots > 0 also the scratch reserved for u_slots extracted
// samples and fenced against its previous user on another stream (released after fn).  Returns
// fn's TFHE_AMD_* code, or the frame's own failure.
struct TfheAmdContext;
int tfhe_amd_internal_frame(TfheAmdContext *c, void *stream, int u_slots,
                            int (*fn)(const tfhe_amd::ContextFrame &, void *), void *arg);
// One blind-rotation batch of B ciphertexts from `in` (one half) in the frame of the device entry
// points of engine.cpp: selected kernel, guard, profile scopes, scratch fence.  res_a set: followed by
// the key switch into (res_a, res_b) through the context's scratch; else the extracted samples go to
// (u_a, u_b).  The caller has checked its arrays; TFHE_AMD_E_ARG for a context without the keys needed.
int tfhe_amd_internal_br_batch(TfheAmdContext *c, void *stream, int B, const tfhe_amd::BrInput *in, int32_t *u_a,
                               int32_t *u_b, int32_t *res_a, int32_t *res_b);
