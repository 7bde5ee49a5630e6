/*
 * tfhe_amd.h — the batched (Tier-2) C ABI of the MI355X gate-bootstrapping engine.
 *
 * It is the throughput path of SURVEY.md §8(b): the reference's bit-coalesced batch API
 * (LweSample_16 = {int* a [B x n], int* b [B]}, gpuParallel/lwesamples.h:9-13) driven
 * by bootsAND_fullGPU_n_Bit / bootsXOR_fullGPU_n_Bit / bootsMUX_fullGPU_n_Bit
 * (gpuParallel/boot-gates.cu:2845-3024) and bootstrapAndKeySwitch_n_Bit (:2481-2629).
 * Each entry point here replaces one of those; unlike the reference, the `b` halves live
 * on the device too, all gates (incl. NAND/OR/NOR/AND-NY..., which the reference GPU
 * path lacks) are supported, and results are Torus32-exact.
 *
 * Plain pointers and sizes only.  Ciphertext batches are SoA:
 *   a : int32 [B][500] (row stride 500), b : int32 [B]
 * `_dev` functions take DEVICE pointers (resident in HBM) and a hipStream_t passed as
 * void* (NULL = the context's own stream); they enqueue and return (call
 * tfhe_amd_sync to wait).  Successive calls on one context may use different streams: the
 * engine orders the reuse of its scratch between them.  A context serves one host thread at
 * a time (the Tier-1 API gives every calling thread its own lane).  `_host` functions take
 * host pointers and are synchronous.
 * A call makes its context's device current only while it runs: the calling thread's current
 * HIP device (the one torch and hipMalloc use) is the same after the call as before.
 * Every function returns 0 on success or a negative TFHE_AMD_E* code.
 */
#ifndef TFHE_AMD_H
#define TFHE_AMD_H

#include <stdint.h>
#include <stddef.h>
#include "tfhe/tfhe_core.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    TFHE_AMD_OK = 0,
    TFHE_AMD_E_ARG = -1,       /* bad argument / unknown gate / B < 0 */
    TFHE_AMD_E_HIP = -2,       /* a HIP runtime call failed */
    TFHE_AMD_E_NODEVICE = -3,  /* no usable GPU / the HIP kernels are not loadable */
    TFHE_AMD_E_NOMEM = -4
};

/* gate codes (boot-gates.cu:98-448) */
enum {
    TFHE_GATE_NAND = 0, TFHE_GATE_OR = 1, TFHE_GATE_AND = 2, TFHE_GATE_XOR = 3,
    TFHE_GATE_XNOR = 4, TFHE_GATE_NOR = 5, TFHE_GATE_ANDNY = 6, TFHE_GATE_ANDYN = 7,
    TFHE_GATE_ORNY = 8, TFHE_GATE_ORYN = 9, TFHE_GATE_MUX = 10,
    /* circuit-only gates (below): */
    TFHE_GATE_MAJ = 11,    /* majority(a, b, c), one bootstrap */
    TFHE_GATE_XOR3 = 12,   /* a ^ b ^ c, one bootstrap */
    TFHE_GATE_NOT = 13,    /* bootsNOT (boot-gates.cu:242): linear, no bootstrap */
    TFHE_GATE_COPY = 14,   /* bootsCOPY: linear */
    TFHE_GATE_CONST = 15   /* bootsCONSTANT: `a` is the bit value, no inputs */
};

typedef struct TfheAmdContext TfheAmdContext;
typedef struct TfheAmdCircuit TfheAmdCircuit;

/* Device context = the key material of one cloud key on one GPU: the bootstrapping key in
 * the kernels' transform domains (converted on the device from the coefficient-domain key) and the
 * key-switching key, plus a stream and scratch.  Replaces the reference's key upload
 * (gpuParallel/main.cu:165-213 sendBootstrappingKeyToGPUCoalesceExt, :236-254, :364-407). */
int tfhe_amd_context_create(const TFheGateBootstrappingCloudKeySet *bk, int device, TfheAmdContext **out);
/* same from raw arrays: bk int32 [500][4][2][1024], ksk int32 [1024][8][4][501] */
int tfhe_amd_context_create_raw(const int32_t *bk, const int32_t *ksk, int device, TfheAmdContext **out);
int tfhe_amd_context_destroy(TfheAmdContext *ctx);
/* A context on `device` holding a copy of src's converted device key, copied device to device
 * (hipMemcpyPeerAsync: xGMI when the GPUs have peer access, staged by HIP otherwise) instead of a
 * host upload and on-device conversion; the multi-device context builds its slots > 0 this way. */
int tfhe_amd_context_create_replica(TfheAmdContext *src, int device, TfheAmdContext **out);
/* FNV-1a 64 of the context's device key bytes (every domain it holds, in a fixed order) */
int tfhe_amd_context_key_digest(TfheAmdContext *ctx, unsigned long long *digest);
int tfhe_amd_context_device(const TfheAmdContext *ctx);
/* device bytes of the context's key material (the transform-domain bootstrapping keys and the
 * key-switching key layouts its kernels read) */
long long tfhe_amd_context_key_bytes(const TfheAmdContext *ctx);
/* the context's stream as a hipStream_t (void*) */
void *tfhe_amd_context_stream(TfheAmdContext *ctx);
int tfhe_amd_sync(TfheAmdContext *ctx);
/* pre-size the scratch for batches of up to B gates (optional; grows on demand otherwise) */
int tfhe_amd_reserve(TfheAmdContext *ctx, int B);

/* B gates; cc_* only for TFHE_GATE_MUX (result = a ? b : c).  res may alias inputs. */
int tfhe_amd_gate_batch_dev(TfheAmdContext *ctx, int gate, int B,
                            int32_t *res_a, int32_t *res_b,
                            const int32_t *ca_a, const int32_t *ca_b,
                            const int32_t *cb_a, const int32_t *cb_b,
                            const int32_t *cc_a, const int32_t *cc_b, void *stream);
int tfhe_amd_gate_batch_host(TfheAmdContext *ctx, int gate, int B,
                             int32_t *res_a, int32_t *res_b,
                             const int32_t *ca_a, const int32_t *ca_b,
                             const int32_t *cb_a, const int32_t *cb_b,
                             const int32_t *cc_a, const int32_t *cc_b);

/* Caller-owned pinned host buffers (page-locked, portable to every device and mapped into every
 * device's address space at the host address; tfhe_amd_host_alloc checks that and returns NULL
 * otherwise).  When every array of a tfhe_amd_gate_batch_host call lies inside buffers from
 * tfhe_amd_host_alloc, the call skips the library's pinned staging: the blind rotation's gate
 * prologue reads the inputs in place over PCIe (zero-copy, no input copy at all), the key switch
 * writes the results to device memory and one DMA per array copies them straight into the caller's
 * arrays, overlapped with the next slice's blind rotation above one round (the reference's per-gate
 * cudaMemcpy pairs, boot-gates.cu:2489-2615, become one DMA per result array).
 * Only the library's own allocations are recognised, so a freed and reused address is never
 * mistaken for pinned memory.  tfhe_amd_host_free returns TFHE_AMD_E_ARG for a pointer that is not
 * the start of a live buffer; tfhe_amd_host_is_pinned reports whether [p, p + bytes) lies in one. */
void *tfhe_amd_host_alloc(size_t bytes);
int tfhe_amd_host_free(void *p);
int tfhe_amd_host_is_pinned(const void *p, size_t bytes);

/* B gates of MIXED kinds (gates[i] = TFHE_GATE_NAND .. TFHE_GATE_MUX, a host array) in one
 * blind-rotation launch and one key-switch launch (a one-level circuit: a MUX is two rows and a
 * combined key switch); cc_* only read for MUX entries (may be NULL without one).  Host arrays,
 * synchronous; res may alias inputs.  The Tier-1 coalescing queue runs its mixed batches
 * through it. */
int tfhe_amd_gate_batch_mixed_host(TfheAmdContext *ctx, int B, const int *gates,
                                   int32_t *res_a, int32_t *res_b,
                                   const int32_t *ca_a, const int32_t *ca_b,
                                   const int32_t *cb_a, const int32_t *cb_b,
                                   const int32_t *cc_a, const int32_t *cc_b);

/* tfhe_bootstrap_woKS_FFT over B inputs x (n=500) -> u (N=1024): u_a [B][1024], u_b [B] */
int tfhe_amd_bootstrap_woks_batch_dev(TfheAmdContext *ctx, int B, int32_t mu,
                                      const int32_t *x_a, const int32_t *x_b,
                                      int32_t *u_a, int32_t *u_b, void *stream);
/* tfhe_bootstrap_FFT over B inputs (woKS + key switch) */
int tfhe_amd_bootstrap_batch_dev(TfheAmdContext *ctx, int B, int32_t mu,
                                 const int32_t *x_a, const int32_t *x_b,
                                 int32_t *res_a, int32_t *res_b, void *stream);
/* lweKeySwitch over B samples u (N=1024) -> res (n=500).
 * ALIGNMENT: u_a must be 16-byte aligned (the key-switch kernels read it 16 bytes at a time; a row is
 * 4096 bytes, so every row then is); a u_a that is not is refused with TFHE_AMD_E_ARG on the host,
 * before any launch.  This is the library's only alignment rule of its own: every other device
 * pointer of every entry point needs 4-byte alignment only (every access to it is a 4-byte access).
 * The host form below stages its input in the library's own scratch and takes any int32 pointer. */
int tfhe_amd_keyswitch_batch_dev(TfheAmdContext *ctx, int B,
                                 const int32_t *u_a, const int32_t *u_b,
                                 int32_t *res_a, int32_t *res_b, void *stream);

/* host-pointer (synchronous) versions of the three above */
int tfhe_amd_bootstrap_woks_batch_host(TfheAmdContext *ctx, int B, int32_t mu,
                                       const int32_t *x_a, const int32_t *x_b,
                                       int32_t *u_a, int32_t *u_b);
int tfhe_amd_bootstrap_batch_host(TfheAmdContext *ctx, int B, int32_t mu,
                                  const int32_t *x_a, const int32_t *x_b,
                                  int32_t *res_a, int32_t *res_b);
int tfhe_amd_keyswitch_batch_host(TfheAmdContext *ctx, int B,
                                  const int32_t *u_a, const int32_t *u_b,
                                  int32_t *res_a, int32_t *res_b);

/* ---- Programmable bootstrapping: a bootstrap that evaluates a caller-supplied
 * function.  The blind rotation starts from ACC = (0, X^{2N - barb} tv) with a test vector tv of
 * N = 1024 Torus32 coefficients instead of the constant (mu, ..., mu) of the sign bootstrap
 * above, so the extracted sample encrypts tv[round(2N phase)] for a phase in [0, 1/2) and
 * -tv[round(2N phase) - N] in [1/2, 1) (the rotation is negacyclic).
 *
 * Encoding convention (tfhe_amd_lut_fill and the Python helpers): a message m in [0, p) sits at
 * the torus value (2m + 1) / (4p), the centre of box m of the p boxes of the half torus [0, 1/2),
 * and tv[j] = values[floor(j p / N)], so box m reads values[m]: a fresh output when the input's
 * phase error stays below 1/(4p).  Table values meant to be looked up again are encoded the same
 * way, values[m] = (2 f(m) + 1) / (4p') as a Torus32.  p must be a power of two in [1, 1024];
 * anything else, or a null pointer, returns TFHE_AMD_E_ARG.  Host only, needs no GPU. */
int tfhe_amd_lut_fill(int32_t tv[1024], int p, const int32_t *values /* [p] */);

/* B programmable bootstraps in one launch.  The blind-rotation input is (0, c) + sa*X + sb*Y (the
 * gate prologue's form; Y is ignored and may be NULL when sb == 0).  tv = n_lut tables of 1024
 * words; ciphertext i takes table lut_index[i] (NULL: table 0).  u = SampleExtract_0 of the rotated
 * accumulator: u_a [B][1024], u_b [B]; the non-woks forms key switch it into res_a [B][500],
 * res_b [B], which may alias X.  All arrays of the _dev forms are on the context's device and the
 * call is asynchronous on `stream` (0: the context's); there the kernel clamps each lut_index entry
 * into [0, n_lut) before it forms an address, so a bad device-side index reads another table but
 * never out of bounds.  The _host forms take host arrays, upload the tables (n_lut x 4 KB) with the
 * inputs, run synchronously and return TFHE_AMD_E_ARG for a lut_index entry outside [0, n_lut).
 * TFHE_AMD_E_ARG also for n_lut <= 0, a null tv and B < 0.  The exactness guard (the flagged
 * ciphertexts are recomputed with the same table), tfhe_amd_select_kernel and
 * tfhe_amd_set_guard_threshold apply as to every other bootstrap; tfhe_amd_last_kernels names the
 * LUT variants, e.g. "k_blind_rotate_v6(lut+reg-rotation)", "k_blind_rotate_v4(lut+guard)". */
int tfhe_amd_bootstrap_lut_woks_batch_dev(TfheAmdContext *ctx, int B, int n_lut, const int32_t *tv,
                                          const int32_t *lut_index, int32_t c, int32_t sa,
                                          const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                          const int32_t *y_a, const int32_t *y_b,
                                          int32_t *u_a, int32_t *u_b, void *stream);
int tfhe_amd_bootstrap_lut_batch_dev(TfheAmdContext *ctx, int B, int n_lut, const int32_t *tv,
                                     const int32_t *lut_index, int32_t c, int32_t sa,
                                     const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                     const int32_t *y_a, const int32_t *y_b,
                                     int32_t *res_a, int32_t *res_b, void *stream);
int tfhe_amd_bootstrap_lut_woks_batch_host(TfheAmdContext *ctx, int B, int n_lut, const int32_t *tv,
                                           const int32_t *lut_index, int32_t c, int32_t sa,
                                           const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                           const int32_t *y_a, const int32_t *y_b,
                                           int32_t *u_a, int32_t *u_b);
int tfhe_amd_bootstrap_lut_batch_host(TfheAmdContext *ctx, int B, int n_lut, const int32_t *tv,
                                      const int32_t *lut_index, int32_t c, int32_t sa,
                                      const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                      const int32_t *y_a, const int32_t *y_b,
                                      int32_t *res_a, int32_t *res_b);

/* ---- Many-LUT bootstrapping: up to nu = 2^log_nu functions of one input from
 * ONE blind rotation (PBS-manyLUT; Chillotti, Ligier, Orfila, Tap 2021).  The modulus switch
 * rounds every mask word and the body to a multiple of nu,
 * bar(x) = ((((uint64)x + 2^(20+log_nu)) >> (21+log_nu)) << log_nu) mod 2N, the 500 CMux steps
 * are the ordinary ones, and the extraction takes the coefficients f = 0 .. n_out-1 of the
 * rotated accumulator instead of only coefficient 0: output f encrypts tv[bar + f] (negacyclic),
 * so a test vector that interleaves the functions, tv[j] = function (j mod nu) at box
 * floor(j p / N), yields function f in output f.  The coarser switch costs margin: the phase
 * error of the switch grows about nu-fold (DESIGN.md §3.3 has the measured figures; p nu <= 16
 * decodes fresh inputs with room to spare).
 *
 * tfhe_amd_lut_fill_many: tv[j] = values[j & (nu-1)][floor(j p / N)] when (j & (nu-1)) < n_fn,
 * else 0; values is [n_fn][p] Torus32.  TFHE_AMD_E_ARG unless p is a power of two,
 * 0 <= log_nu <= 4, 1 <= n_fn <= nu, p nu <= 1024 and the pointers are non-null (tv is then
 * untouched).  log_nu = 0, n_fn = 1 is tfhe_amd_lut_fill.  Host only, needs no GPU. */
int tfhe_amd_lut_fill_many(int32_t tv[1024], int p, int log_nu, int n_fn, const int32_t *values /* [n_fn][p] */);

/* The batch forms: the arguments of the tfhe_amd_bootstrap_lut_* function of the same name with
 * log_nu, n_out after lut_index.  Outputs are function-major, u_a [n_out][B][1024], u_b [n_out][B]
 * and res_a [n_out][B][500], res_b [n_out][B], so each function's block is an ordinary batch for
 * the next call; the key-switched forms run one key switch over the n_out B samples, and res may
 * alias X.  Everything said of the single-table forms holds (lut_index clamped on the device and
 * checked on the host, guard, tfhe_amd_select_kernel, asynchronous _dev forms).  The exactness
 * guard is per ciphertext: a flagged one is recomputed exactly with the same log_nu and table and
 * all its n_out outputs rewritten; tfhe_amd_guard_stats counts ciphertexts.  TFHE_AMD_E_ARG
 * additionally for log_nu outside [0, 4] or n_out outside [1, 2^log_nu].  tfhe_amd_last_kernels
 * says "lut-many" where the single-table launches say "lut", e.g.
 * "k_blind_rotate_v6(lut-many+reg-rotation)", "k_blind_rotate_v4(lut-many+guard)". */
int tfhe_amd_bootstrap_lut_many_woks_batch_dev(TfheAmdContext *ctx, int B, int n_lut, const int32_t *tv,
                                               const int32_t *lut_index, int log_nu, int n_out,
                                               int32_t c, int32_t sa,
                                               const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                               const int32_t *y_a, const int32_t *y_b,
                                               int32_t *u_a, int32_t *u_b, void *stream);
int tfhe_amd_bootstrap_lut_many_batch_dev(TfheAmdContext *ctx, int B, int n_lut, const int32_t *tv,
                                          const int32_t *lut_index, int log_nu, int n_out,
                                          int32_t c, int32_t sa,
                                          const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                          const int32_t *y_a, const int32_t *y_b,
                                          int32_t *res_a, int32_t *res_b, void *stream);
int tfhe_amd_bootstrap_lut_many_woks_batch_host(TfheAmdContext *ctx, int B, int n_lut, const int32_t *tv,
                                                const int32_t *lut_index, int log_nu, int n_out,
                                                int32_t c, int32_t sa,
                                                const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                                const int32_t *y_a, const int32_t *y_b,
                                                int32_t *u_a, int32_t *u_b);
int tfhe_amd_bootstrap_lut_many_batch_host(TfheAmdContext *ctx, int B, int n_lut, const int32_t *tv,
                                           const int32_t *lut_index, int log_nu, int n_out,
                                           int32_t c, int32_t sa,
                                           const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                           const int32_t *y_a, const int32_t *y_b,
                                           int32_t *res_a, int32_t *res_b);

/* One-rotation full adders in a batch (the encodings, the cell and the circuit
 * builders: below, at tfhe_amd_circuit_full_add).  B independent cells: a, b and c hold one
 * half-torus bit (TFHE_AMD_ENC_HALF) per cell, c_a = c_b = NULL makes half adders.  One many-LUT
 * launch over the three inputs, (0, -(k - 1)/16) + a + b (+ c) with k the number of inputs, and
 * one key switch over the 2 B samples; results are function-major like
 * tfhe_amd_bootstrap_lut_many_batch_*: res_a [2][B][500], res_b [2][B], block 0 the sum bits in
 * enc_sum, block 1 the carries in enc_carry.  res may alias an input.  The entry for callers who
 * schedule their own levels (a vector adder: one call per bit position).  The context keeps the
 * four tables on its device (16 KB, made at the first call, freed with the context; not key
 * material: tfhe_amd_context_key_digest / _key_bytes do not see them).  The _dev form is
 * asynchronous on `stream`; the _host form stages through the context's buffers and is
 * synchronous.  Guard, tfhe_amd_select_kernel and tfhe_amd_last_kernels as for the many-LUT
 * forms ("lut-many" launches).  TFHE_AMD_E_ARG for an unknown encoding, B < 0, a null a, b or res
 * and for exactly one of c_a, c_b null.  The library cannot check that the inputs are H bits. */
int tfhe_amd_full_add_batch_dev(TfheAmdContext *ctx, int B, int enc_sum, int enc_carry,
                                const int32_t *a_a, const int32_t *a_b, const int32_t *b_a, const int32_t *b_b,
                                const int32_t *c_a, const int32_t *c_b, int32_t *res_a, int32_t *res_b,
                                void *stream);
int tfhe_amd_full_add_batch_host(TfheAmdContext *ctx, int B, int enc_sum, int enc_carry,
                                 const int32_t *a_a, const int32_t *a_b, const int32_t *b_a, const int32_t *b_b,
                                 const int32_t *c_a, const int32_t *c_b, int32_t *res_a, int32_t *res_b);

/* Debug/parity entry: run `iters` CMux steps of the blind rotation (i = 0..iters-1,
 * tfhe_MuxRotate_FFT, skipping bara_i == 0 like tfhe_blindRotate_FFT) on B explicit
 * accumulators acc [B][2][1024] in place, with rotations bara [B][iters].  The raw steps of the
 * selected kernel generation, WITHOUT the exactness guard (the fp64 kernel's roundings are not
 * checked): a kernel-test entry.  The exact L1 function is tfhe_blindRotate_FFT (tfhe.h). */
int tfhe_amd_blind_rotate_dev(TfheAmdContext *ctx, int B, int iters, int32_t *acc,
                              const int32_t *bara, void *stream);
/* tGswFFTExternMulToTLwe (tgsw_functions.h:70, tgsw-fft-operations.cu:124-264) on B accumulators:
 * acc [B][2][1024] <- BK_i (x) acc with i = key_index[b] (device arrays), exact (the NTT kernel's
 * arithmetic); the reference replaces the accumulator by the product the same way.  An index
 * outside [0, 500) leaves its accumulator unchanged (checked on the device). */
int tfhe_amd_external_product_dev(TfheAmdContext *ctx, int B, const int32_t *key_index, int32_t *acc,
                                  void *stream);

/* ---- Leveled mode: CMux chains on caller-supplied TGSW ciphertexts.
 * Every bootstrap costs 500 CMux steps on the 500 TGSW samples of the bootstrapping key.  When the
 * CLIENT supplies the address bits of a table lookup as TGSW ciphertexts, a lookup in a table of
 * 2^d entries is d CMux steps: with the table in a polynomial, step i multiplies the accumulator by
 * X^{-2^i} when bit i is 1, and sample extraction reads the entry at coefficient 0.  The output
 * carries about the noise of a gate's output before its key switch; after the key switch it is an
 * ordinary n = 500 sample that every gate, LUT row and full_add cell can read.
 * LIMIT: the address bits must arrive as TGSW ciphertexts from the client.  A computed LWE bit
 * cannot be turned into one (that is circuit bootstrapping, which this library does not have), so
 * this serves the input layer of a computation: S-boxes, ROMs, private reads on client indices.
 * The TABLE has no such limit: besides a plaintext polynomial or a client's encryption
 * (tfhe_amd_tlwe_encrypt_polys) an encrypted table can come from tfhe_amd_pack_* below, which gathers
 * up to 1024 computed LWE samples into one TLWE ciphertext on the device.
 *
 * Client side (host only, no GPU; both draw from the library's generator, so
 * tfhe_random_generator_setSeed makes them reproducible):
 * tfhe_amd_tgsw_encrypt_bits: n TGSW encryptions of bits[i] in {0, 1} under the keyset's TGSW key
 *   at its alpha_min, exactly as key generation encrypts the LWE key bits; out is
 *   int32 [n][4][2][1024], the layout of one entry of tfhe_amd_export_bk (row, then a / b).
 * tfhe_amd_tlwe_encrypt_polys: n TLWE encryptions of the message polynomials mu [n][1024] under
 *   the same key and noise, out [n][2][1024] (a, then b): encrypted tables.
 * TFHE_AMD_E_ARG for a null pointer, n < 0 or a bit outside {0, 1} (nothing is drawn then). */
int tfhe_amd_tgsw_encrypt_bits(const TFheGateBootstrappingSecretKeySet *key, int n, const int32_t *bits,
                               int32_t *out);
int tfhe_amd_tlwe_encrypt_polys(const TFheGateBootstrappingSecretKeySet *key, int n, const int32_t *mu,
                                int32_t *out);

/* An imported set: n coefficient-domain TGSW samples (host, [n][4][2][1024]) uploaded to the
 * context's device and converted there into the exact kernels' layout (two 27-bit primes, 64 KB per
 * sample).  Synchronous.  The set lives on that device and does not depend on the context's
 * lifetime; it may be used with any context on the same device (also a key-switch-only one for the
 * woks forms), and a call that pairs it with a context on another device returns TFHE_AMD_E_ARG.
 * Destroy waits for the device.  count: the number of samples, or TFHE_AMD_E_ARG for NULL. */
typedef struct TfheAmdTgsw TfheAmdTgsw;
int tfhe_amd_tgsw_import(TfheAmdContext *ctx, int n, const int32_t *coef_host, TfheAmdTgsw **out);
int tfhe_amd_tgsw_count(const TfheAmdTgsw *set);
int tfhe_amd_tgsw_destroy(TfheAmdTgsw *set);

/* B CMux gates on TLWE samples [B][2][1024] (a, then b; device arrays, asynchronous):
 * out[w] = d0[w] + C (x) (d1[w] - d0[w]) with C sample sel[w] of the set, i.e. d1 where C encrypts
 * 1 and d0 where it encrypts 0, exact arithmetic.  d0 = NULL: the plain external product
 * C (x) d1[w].  out may be d0 or d1 (the same array; other overlaps are not supported).  sel is a
 * device array: an index outside [0, count) gives out[w] = d0[w] (zero for d0 = NULL), checked on
 * the device before any address is formed. */
int tfhe_amd_tgsw_cmux_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, int B, const int32_t *sel,
                           const int32_t *d1, const int32_t *d0, int32_t *out, void *stream);

/* B table lookups.  Query q reads table t = tab_index[q] (NULL: table 0) at the d-bit address
 * addr = sum_i bit_i 2^i whose bit i is encrypted by sample sel[q * d + i] of the set (bit 0
 * first; queries may share samples).
 *   tab: int32 [n_tab][n_poly][tab_rows][1024].  tab_rows = 1: plaintext polynomials of Torus32
 *     entries (the trivial sample (0, tab)); tab_rows = 2: TLWE samples (a, then b) from
 *     tfhe_amd_tlwe_encrypt_polys.
 *   Horizontal packing: a polynomial holds 2^d_h entries of 2^log_stride words each, entry e at
 *     the coefficients e << log_stride ..., and output f < n_out encrypts
 *     tab[t][(addr_h << log_stride) + f].  d_h + log_stride <= 10, 1 <= n_out <= min(16, 2^log_stride).
 *   Vertical packing: n_poly in {1, 2, 4, 8, 16} polynomials per table and d = d_h + log2(n_poly);
 *     the address bits d_h .. d - 1 pick the polynomial through a CMux tree (bit d_h pairs the
 *     polynomials 2 j, 2 j + 1), one k_tgsw_cmux_v4 launch per level, then the rotation kernel runs
 *     on the tree's result.  The tree's scratch belongs to the set and grows on demand.
 * Outputs are function-major like tfhe_amd_bootstrap_lut_many_*: the woks forms return the
 * extracted samples u_a [n_out][B][1024], u_b [n_out][B] under the extracted TLWE key; the other
 * forms run ONE key switch over the n_out B samples and return res_a [n_out][B][500],
 * res_b [n_out][B].  The _dev forms take device arrays and are asynchronous on `stream`; a
 * selector index outside [0, count) skips its CMux step and a tab_index entry is clamped into
 * [0, n_tab), both on the device before any address is formed.  The _host forms take host arrays,
 * stage through temporary device buffers, are synchronous and return TFHE_AMD_E_ARG for any
 * selector index outside [0, count) or tab_index entry outside [0, n_tab).  TFHE_AMD_E_ARG also
 * for a shape outside the limits above, a null array, and a context without key-switching key in
 * the key-switched forms.
 * There is no fp64 form of these kernels: tfhe_amd_select_kernel and the exactness guard do not
 * apply, the arithmetic is always the exact two-prime NTT.  tfhe_amd_last_kernels reports, in
 * launch order, "k_tgsw_cmux_v4(tree-level-0)", ... once per tree level, "k_tgsw_lookup_v4" and the
 * key switch's own name; tfhe_amd_tgsw_cmux_dev reports "k_tgsw_cmux_v4". */
int tfhe_amd_tgsw_lookup_woks_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, int B, int d, const int32_t *sel,
                                  int n_tab, int n_poly, int tab_rows, const int32_t *tab,
                                  const int32_t *tab_index, int log_stride, int n_out,
                                  int32_t *u_a, int32_t *u_b, void *stream);
int tfhe_amd_tgsw_lookup_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, int B, int d, const int32_t *sel,
                             int n_tab, int n_poly, int tab_rows, const int32_t *tab,
                             const int32_t *tab_index, int log_stride, int n_out,
                             int32_t *res_a, int32_t *res_b, void *stream);
int tfhe_amd_tgsw_lookup_woks_host(TfheAmdContext *ctx, TfheAmdTgsw *set, int B, int d, const int32_t *sel,
                                   int n_tab, int n_poly, int tab_rows, const int32_t *tab,
                                   const int32_t *tab_index, int log_stride, int n_out,
                                   int32_t *u_a, int32_t *u_b);
int tfhe_amd_tgsw_lookup_host(TfheAmdContext *ctx, TfheAmdTgsw *set, int B, int d, const int32_t *sel,
                              int n_tab, int n_poly, int tab_rows, const int32_t *tab,
                              const int32_t *tab_index, int log_stride, int n_out,
                              int32_t *res_a, int32_t *res_b);

/* ---- Leveled automata: a deterministic automaton over client TGSW bits.
 * The other leveled primitive: an automaton of Q states, a start state and transitions
 * next[s * 2 + bit] reads a word of len bits that arrive as TGSW ciphertexts, at one exact CMux per
 * live state and input bit and no bootstrap.  A function that reads its input bit-serially (compare
 * two integers, find a pattern, count flags up to a threshold) is evaluated that way; the result is,
 * after the key switch, an ordinary n = 500 sample that every gate, LUT row and select node can read.
 * The same LIMIT as the lookup's: the bits must be the client's TGSW ciphertexts.
 *
 * Semantics.  Query q reads bit i (bit 0 first) from sample sel[q * len + i] of the set.  The final
 * weights fin [n_fin][Q][fin_rows][1024] hold one polynomial per state (fin_rows = 1: plaintext
 * Torus32 words, the trivial sample (0, fin); fin_rows = 2: TLWE samples (a, then b) from
 * tfhe_amd_tlwe_encrypt_polys or tfhe_amd_pack_*); query q uses table fin_index[q] (NULL: table 0).
 * The evaluation runs backwards over the word: ACC_len[s] = fin[s], and for j = len .. 1
 *   ACC_{j-1}[s] = d0 + C_j (x) (d1 - d0 + 2^11 (1 + X + ... + X^1023) on both polynomials)
 * with d_b = ACC_j[next[s][b]] and C_j the sample of bit j - 1, the exact product of the CMux gate.
 * The 2^11 centres the gadget decomposition's truncation, whose mean would otherwise add up along
 * the chain; the product reads only the digits, so nothing else changes.  The
 * output ACC_0[start] has the phase fin[state reached after the whole word] plus noise; its
 * coefficients 0 .. n_out - 1 (n_out <= 16) are extracted, function-major as in the lookup: the woks
 * forms return u_a [n_out][B][1024], u_b [n_out][B], the other forms run ONE key switch over the
 * n_out B samples into res_a [n_out][B][500], res_b [n_out][B].
 * Step j computes only the states reachable from the start state after j - 1 bits (the live sets
 * R_{j-1}, computed once at creation), and a state with next0 == next1 copies its operand: its
 * product is exactly zero.
 *
 * tfhe_amd_dfa_create: an automaton on the context's device: the transitions and the live sets
 *   R_0 .. R_{max_len - 1} uploaded once, and the state scratch of the runs (two buffers of Q TLWE
 *   samples per query, grown on demand, at most 256 MiB: a larger batch runs in slices), shared by the
 *   runs on the automaton and ordered across streams like a set's tree scratch.  Like a set it does
 *   not depend on the context's lifetime and may be used with any context on the same device.
 *   ctx = NULL makes a host-only automaton (device -1) that _info and _live read and every run
 *   refuses; it touches no device.  1 <= n_states <= 64, 0 <= start < n_states, 1 <= max_len <= 1024
 *   (one product adds a variance of 4 * 1024 * (2^20 / 12) * sigma_bk^2 = 1.85e-8, so 1024 steps give
 *   a standard deviation of 4.4e-3, 1/32 over 7), every transition in [0, n_states); else
 *   TFHE_AMD_E_ARG and *out = NULL.  Destroy waits for the device and takes NULL.
 * tfhe_amd_dfa_info: any of n_states, start, max_len, device may be NULL.
 * tfhe_amd_dfa_live: the number of states of R_step, 0 <= step <= max_len, written in ascending
 *   order to states (at most n_states words; NULL: the count alone); TFHE_AMD_E_ARG otherwise.
 *
 * tfhe_amd_dfa_run_*: B queries of len bits, 1 <= len <= max_len.  The _dev forms take device arrays
 * and are asynchronous on `stream`; every index they read is checked on the device before an address
 * is formed: a selector outside [0, count) gives that step's result = the next[s][0] operand, a
 * fin_index entry is clamped into [0, n_fin).  The _host forms stage through temporary device
 * buffers, are synchronous and return TFHE_AMD_E_ARG for any selector or fin_index entry out of
 * range, writing nothing.  TFHE_AMD_E_ARG also for B < 0, len outside [1, max_len], n_fin < 1,
 * fin_rows outside {1, 2}, n_out outside [1, 16], null arrays with B > 0, a set or automaton on
 * another device than the context's and, in the key-switched forms, a context without
 * key-switching key; B = 0 returns TFHE_AMD_OK.
 * There is no fp64 form: tfhe_amd_select_kernel and the exactness guard do not apply.
 * There is one launch per input bit; tfhe_amd_last_kernels reports (each name once, in launch order)
 * "k_tgsw_dfa_v4(weights)" for the last bit (it reads the final weights), "k_tgsw_dfa_v4" for the
 * bits in between and "k_tgsw_dfa_v4(extract)" for bit 0 (it extracts the start state's result);
 * len = 1 is the single launch "k_tgsw_dfa_v4(weights+extract)"; then the key switch's own name. */
typedef struct TfheAmdDfa TfheAmdDfa;
int tfhe_amd_dfa_create(TfheAmdContext *ctx, int n_states, int start, const int32_t *next, int max_len,
                        TfheAmdDfa **out);
int tfhe_amd_dfa_destroy(TfheAmdDfa *dfa);
int tfhe_amd_dfa_info(const TfheAmdDfa *dfa, int *n_states, int *start, int *max_len, int *device);
int tfhe_amd_dfa_live(const TfheAmdDfa *dfa, int step, int32_t *states);
int tfhe_amd_dfa_run_woks_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                              const int32_t *sel, int n_fin, int fin_rows, const int32_t *fin,
                              const int32_t *fin_index, int n_out, int32_t *u_a, int32_t *u_b, void *stream);
int tfhe_amd_dfa_run_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                         const int32_t *sel, int n_fin, int fin_rows, const int32_t *fin,
                         const int32_t *fin_index, int n_out, int32_t *res_a, int32_t *res_b, void *stream);
int tfhe_amd_dfa_run_woks_host(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                               const int32_t *sel, int n_fin, int fin_rows, const int32_t *fin,
                               const int32_t *fin_index, int n_out, int32_t *u_a, int32_t *u_b);
int tfhe_amd_dfa_run_host(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                          const int32_t *sel, int n_fin, int fin_rows, const int32_t *fin,
                          const int32_t *fin_index, int n_out, int32_t *res_a, int32_t *res_b);

/* Builders (host only, no GPU): they fill next [n_states][2] and *start and return the number of
 * states, or TFHE_AMD_E_ARG for a null pointer or a parameter outside its range.
 * tfhe_amd_dfa_build_compare: x against y over the word x_{d-1}, y_{d-1}, ..., x_0, y_0 (most
 *   significant pair first, any d: len = 2 d): 5 states, next [5][2]; cls [5] (may be NULL) gets the
 *   class of each state, after a whole number of pairs x < y, x = y or x > y, or between the two
 *   bits of a pair.
 * tfhe_amd_dfa_build_contains: the Knuth-Morris-Pratt automaton of the pattern of m bits
 *   (pattern[0] is read first), 1 <= m <= 63: m + 1 states, next [m + 1][2]; state k = the longest
 *   prefix of the pattern that ends the word read so far, state m absorbing: the word contains the
 *   pattern.
 * tfhe_amd_dfa_build_at_least: a saturating count of the ones up to t, 1 <= t <= 63: t + 1 states,
 *   next [t + 1][2], state t absorbing: at least t bits are set.
 * tfhe_amd_dfa_fin_fill: fin [n_states][1024] (one table at fin_rows = 1) with values
 *   [n_states][n_out] at the coefficients 0 .. n_out - 1 of each state and zeros elsewhere,
 *   1 <= n_out <= 16; returns TFHE_AMD_OK.
 * tfhe_amd_dfa_simulate: the state after the plain word bits [len] (bit 0 first, len >= 0), or
 *   TFHE_AMD_E_ARG for a bit outside {0, 1}, a transition outside [0, n_states) and bad shapes. */
enum { TFHE_AMD_DFA_LT = 0, TFHE_AMD_DFA_EQ = 1, TFHE_AMD_DFA_GT = 2, TFHE_AMD_DFA_MID = 3 };
int tfhe_amd_dfa_build_compare(int32_t *next, int *start, int32_t *cls);
int tfhe_amd_dfa_build_contains(int m, const int32_t *pattern, int32_t *next, int *start);
int tfhe_amd_dfa_build_at_least(int t, int32_t *next, int *start);
int tfhe_amd_dfa_fin_fill(int n_states, int n_out, const int32_t *values, int32_t *fin);
int tfhe_amd_dfa_simulate(int n_states, int start, const int32_t *next, int len, const int32_t *bits);

/* ---- Weighted runs of a leveled automaton: every transition adds a plaintext
 * monomial to the accumulator, so a run returns values computed from the word and not only a class of
 * it.  The automaton is a TfheAmdDfa as above; a run takes two more arrays, shared by its queries:
 *   w_val [n_states][2]: a Torus32 scalar per (state, bit);
 *   w_pos [len]: the coefficient position of step i, in [0, 1024).
 * For j = len .. 1, i = j - 1, p = w_pos[i] and every state s of R_{j-1}:
 *   d_b = ACC_j[next[s][b]] + (0, w_val[s][b] X^p)   (the b polynomial's coefficient p alone)
 *   ACC_{j-1}[s] = d0 + C_i (x) (d1 - d0 + 2^11 on every word)
 * so the phase of ACC_0[start] is fin[s_len] + sum_i w_val[s_i][bit_i] X^{w_pos[i]} plus noise, s_i
 * the state before bit i is read.  The weights are plaintext and add no noise.  A state copies its
 * operand (d0 + w0 X^p) only when next0 == next1 and w0 == w1; a selector outside [0, count) gives
 * d0 + w0 X^p too.  All-zero w_val gives exactly the words of tfhe_amd_dfa_run_*.
 *
 * tfhe_amd_wfa_run_*: the arguments, layouts, slicing, ordering and refusals of the tfhe_amd_dfa_run_*
 * form of the same suffix, with w_val and w_pos behind sel (device arrays in the _dev forms, host
 * arrays in the _host forms) and n_out in [1, 64].  Null weight arrays with B > 0 are refused.  In the
 * _dev forms a w_pos[i] outside [0, 1024) makes step i weightless (both weights count as 0); the
 * _host forms return TFHE_AMD_E_ARG for it and write nothing.
 * tfhe_amd_last_kernels reports "k_tgsw_dfa_v4(weights+tw)" for the last bit, "k_tgsw_dfa_v4(tw)" for
 * the bits in between, "k_tgsw_dfa_v4(tw+extract)" for bit 0 and "k_tgsw_dfa_v4(weights+tw+extract)"
 * for len = 1; then the key switch's own name. */
int tfhe_amd_wfa_run_woks_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                              const int32_t *sel, const int32_t *w_val, const int32_t *w_pos, int n_fin,
                              int fin_rows, const int32_t *fin, const int32_t *fin_index, int n_out, int32_t *u_a,
                              int32_t *u_b, void *stream);
int tfhe_amd_wfa_run_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                         const int32_t *sel, const int32_t *w_val, const int32_t *w_pos, int n_fin, int fin_rows,
                         const int32_t *fin, const int32_t *fin_index, int n_out, int32_t *res_a, int32_t *res_b,
                         void *stream);
int tfhe_amd_wfa_run_woks_host(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                               const int32_t *sel, const int32_t *w_val, const int32_t *w_pos, int n_fin,
                               int fin_rows, const int32_t *fin, const int32_t *fin_index, int n_out, int32_t *u_a,
                               int32_t *u_b);
int tfhe_amd_wfa_run_host(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                          const int32_t *sel, const int32_t *w_val, const int32_t *w_pos, int n_fin, int fin_rows,
                          const int32_t *fin, const int32_t *fin_index, int n_out, int32_t *res_a, int32_t *res_b);

/* Weighted builders (host only, no GPU): they fill next [n_states][2], *start, w_val [n_states][2] and
 * w_pos [len] and return the number of states, or TFHE_AMD_E_ARG for a null pointer or a parameter
 * outside its range.
 * tfhe_amd_wfa_build_max: max(x, y) (want_max != 0) or min(x, y) of two d-bit integers, 1 <= d <= 64,
 *   over the word x_{d-1}, y_{d-1}, ..., x_0, y_0 (len = 2 d): 7 states, next and w_val [7][2], w_pos
 *   [2 d].  State 0: equal so far; 1 / 2: equal so far and this pair's x bit read, 0 / 1; 3 / 4: x < y
 *   decided and an x / a y bit comes next; 5 / 6: x > y decided likewise (w_val does not depend on the
 *   position, so the decided states tell an x bit from a y bit).  The weight is 2^30 on exactly the
 *   transitions where the result's bit is 1, at coefficient d - 1 - k for the k-th pair read (bit
 *   d - 1 - k of the integers).  With fin = -2^29 at the coefficients 0 .. d - 1 of every state
 *   (tfhe_amd_wfa_fin_fill) output f is bit f of the result in the gate encoding +-1/8, n_out = d.
 *   At most 5 products per pair.
 * tfhe_amd_wfa_build_popcount: the number of set bits of a word of len bits as a LUT digit modulo p,
 *   p in {2, 4, 8, 16}, 1 <= len <= p - 1: one state, w_val[0][1] = 2^32 / (2 p), every w_pos = 0.
 *   With fin = 2^32 / (4 p) at coefficient 0 the single output is the digit (2 c + 1) / (4 p) of the
 *   count c, an input of tfhe_amd_bootstrap_lut_*.
 * tfhe_amd_wfa_build_first_one: the one-hot position of the first set bit of a word of len bits,
 *   1 <= len <= 64: two states (0: none seen, 1: seen, absorbing), w_val[0][1] = 2^30, w_pos[i] = i.
 *   With fin = -2^29 at the coefficients 0 .. len - 1 output f is 1 exactly when bit f is the first
 *   set bit, in the gate encoding, n_out = len.
 * tfhe_amd_wfa_fin_fill: fin [n_states][1024] with `value` at the coefficients 0 .. n_out - 1 of
 *   every state and zeros elsewhere, 1 <= n_out <= 64; returns TFHE_AMD_OK.
 * tfhe_amd_wfa_simulate: poly [1024] = sum_i w_val[s_i][bits[i]] X^{w_pos[i]} (wrapping) for the plain
 *   word bits [len] (bit 0 first, len >= 0); returns the final state, or TFHE_AMD_E_ARG for a bit
 *   outside {0, 1}, a w_pos entry outside [0, 1024), a transition outside [0, n_states) and bad
 *   shapes, with poly untouched. */
int tfhe_amd_wfa_build_max(int d, int want_max, int32_t *next, int *start, int32_t *w_val, int32_t *w_pos);
int tfhe_amd_wfa_build_popcount(int len, int p, int32_t *next, int *start, int32_t *w_val, int32_t *w_pos);
int tfhe_amd_wfa_build_first_one(int len, int32_t *next, int *start, int32_t *w_val, int32_t *w_pos);
int tfhe_amd_wfa_fin_fill(int n_states, int n_out, int32_t value, int32_t *fin);
int tfhe_amd_wfa_simulate(int n_states, int start, const int32_t *next, const int32_t *w_val, const int32_t *w_pos,
                          int len, const int32_t *bits, int32_t *poly);

/* ---- Packing key switch: computed LWE samples gathered into TLWE ciphertexts.
 * The public functional key switch with f = identity onto coefficient positions: P <= 1024 samples
 * (a_p, b_p) under the n = 500 LWE key become ONE TLWE ciphertext under the keyset's TLWE key whose
 * phase b - a s has, at coefficient pos[p], the phase of input p plus noise, and 0 plus noise at
 * every unoccupied coefficient.  Two uses: a table for tfhe_amd_tgsw_lookup_* (tab_rows = 2) made of
 * values the server computed, and result compression (1024 results in one 8 KB ciphertext that the
 * client reads with one phase computation).  Arithmetic: base 2^4, 6 balanced digits in [-8, 7] of
 * every mask word (24 bits), OUT = (0, sum_p b_p X^pos[p]) - sum_{i,j} D_ij (*) K_ij with
 * D_ij = sum_p d_j(a_p[i]) X^pos[p], exact mod 2^32.  The added noise has the standard deviation
 * sqrt(500 * 6 * 21.5 * P) * 7.18e-9 of the torus, 5.8e-5 at P = 1024.
 *
 * Client side (host only, no GPU):
 * tfhe_amd_pack_key_generate: the key, int32 [500][6][2][1024] (24.6 MB): row (i, j) is a TLWE
 *   encryption (a, then b) of the constant polynomial s_i 2^(32 - 4 j), j = 1 .. 6, under the
 *   keyset's TLWE key at its alpha_min.  It draws from the library's generator, rows in (i, j)
 *   order, so tfhe_random_generator_setSeed makes it reproducible.
 * tfhe_amd_tlwe_phase_polys: phase [n][1024] = b - a s mod 2^32 of n TLWE samples in [n][2][1024]:
 *   the client's read of packed results.
 * Both return TFHE_AMD_E_ARG for a null pointer and for n < 0. */
int tfhe_amd_pack_key_generate(const TFheGateBootstrappingSecretKeySet *key, int32_t *out);
int tfhe_amd_tlwe_phase_polys(const TFheGateBootstrappingSecretKeySet *key, int n, const int32_t *in,
                              int32_t *phase);

/* The imported key: uploaded to the context's device and converted there into the exact kernels'
 * layout (48 MB).  Synchronous.  Like a TfheAmdTgsw it lives on that device, does not depend on the
 * context's lifetime and may be used with any context on the same device; pairing it with a
 * context on another device returns TFHE_AMD_E_ARG.  It owns the digit scratch of the pack calls
 * (2 MB per output of the largest batch so far, at most 512 outputs' worth; grown on demand).
 * Destroy waits for the device. */
typedef struct TfheAmdPackKey TfheAmdPackKey;
int tfhe_amd_pack_key_import(TfheAmdContext *ctx, const int32_t *coef_host, TfheAmdPackKey **out);
int tfhe_amd_pack_key_destroy(TfheAmdPackKey *key);

/* T output ciphertexts of P inputs each: in_a [T][P][500], in_b [T][P], out [T][2][1024] (a, then
 * b); pos [P] (shared by the T outputs; NULL: pos[p] = p) gives the distinct coefficient positions.
 * A function-major many-LUT result [n_out][B][500] or a gate batch packs in place with T = n_out,
 * P = B.  tfhe_amd_pack_dev takes device arrays and is asynchronous on `stream`; tfhe_amd_pack_host
 * takes host arrays, stages through temporary device buffers and is synchronous.
 * TFHE_AMD_E_ARG for T < 0, P outside [1, 1024] with T > 0, a null array, a null key or context and
 * a context on another device than the key's; T = 0 returns TFHE_AMD_OK.  The host form also
 * refuses a pos entry outside [0, 1024) and duplicate positions, and writes no output then.  The
 * device form checks every pos entry on the device before any address is formed from it: an entry
 * outside [0, 1024) drops that input (for the whole launch alike); duplicate positions are the
 * caller's error and leave that output ciphertext unspecified, with nothing read or written out of
 * bounds.
 * There is no fp64 form: tfhe_amd_select_kernel and the exactness guard do not apply, the
 * arithmetic is always the exact two-prime NTT.  tfhe_amd_last_kernels reports "k_pack_digits" and
 * then "k_pack_v4(split)" when each output's key rows are split over several workgroups (T at most
 * the device's compute units), else "k_pack_v4". */
int tfhe_amd_pack_dev(TfheAmdContext *ctx, TfheAmdPackKey *key, int T, int P, const int32_t *in_a,
                      const int32_t *in_b, const int32_t *pos, int32_t *out, void *stream);
int tfhe_amd_pack_host(TfheAmdContext *ctx, TfheAmdPackKey *key, int T, int P, const int32_t *in_a,
                       const int32_t *in_b, const int32_t *pos, int32_t *out);

/* ---- Bootstrap from encrypted accumulators: a computed digit selects among
 * computed values.  Every other bootstrap starts its blind rotation from a trivial sample
 * (0, X^-bar(b) tv) with a plaintext tv; these start from X^-bar(b) (A, B), a TLWE ciphertext the
 * server made itself (tfhe_amd_pack_* and the box fill below), so the selector's digit picks a
 * coefficient of a table of computed values: the second level of tree-based programmable
 * bootstrapping.  The 500 CMux steps, the exactness guard (a flagged ciphertext is recomputed from the
 * same accumulator), tfhe_amd_select_kernel and the extraction at coefficient 0 are those of every
 * bootstrap; the output's noise is the accumulator's plus a blind rotation's.
 *
 * tfhe_amd_tlwe_box_fill_*: out = in (1 + X + ... + X^(w-1)), w = 2^log_w, on both polynomials of T
 * TLWE samples [T][2][1024], negacyclic and exact mod 2^32: out[j] = sum_{k<w} +-in[(j-k) mod 1024],
 * minus where j - k < 0.  A sample packed with value m at coefficient m w (and nothing between the
 * occupied positions) then carries value m over the whole box [m w, (m+1) w) of the LUT convention,
 * which is what a rotation by a noisy selector needs.  out may be in; log_w = 0 is a copy.
 * TFHE_AMD_E_ARG for T < 0, log_w outside [0, 10] and null arrays with T > 0.  Trace name
 * "k_tlwe_box_fill". */
int tfhe_amd_tlwe_box_fill_dev(TfheAmdContext *ctx, int T, int log_w, const int32_t *in, int32_t *out,
                               void *stream);
int tfhe_amd_tlwe_box_fill_host(TfheAmdContext *ctx, int T, int log_w, const int32_t *in, int32_t *out);

/* B bootstraps from the accumulators acc [n_acc][2][1024] (a, then b).  The selector is
 * (0, c) + sa*X + sb*Y as in the LUT forms (Y ignored, may be NULL, when sb == 0); ciphertext i starts
 * from accumulator acc_index[i]; acc_index = NULL means accumulator 0 when n_acc == 1 and accumulator
 * i when n_acc == B, and is TFHE_AMD_E_ARG for any other n_acc.  The woks forms return
 * SampleExtract_0 of the rotated accumulator, u_a [B][1024], u_b [B]; the others key switch it into
 * res_a [B][500], res_b [B].  No output may alias acc (the guard's recomputation reads it again);
 * res may alias X.  The _dev forms take device arrays and are asynchronous on `stream`; the kernel
 * clamps each acc_index entry into [0, n_acc) before it forms an address.  The _host forms stage
 * through temporary device buffers, are synchronous and return TFHE_AMD_E_ARG for an acc_index entry
 * outside [0, n_acc), writing nothing.  TFHE_AMD_E_ARG also for n_acc <= 0, B < 0, null arrays and,
 * in the key-switched forms, a context without key-switching key.  tfhe_amd_last_kernels names the
 * variants with "tlwe" where the LUT forms say "lut", e.g. "k_blind_rotate_v6(tlwe+reg-rotation)",
 * "k_blind_rotate_v4(tlwe+guard)". */
int tfhe_amd_bootstrap_acc_woks_batch_dev(TfheAmdContext *ctx, int B, int n_acc, const int32_t *acc,
                                          const int32_t *acc_index, int32_t c, int32_t sa,
                                          const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                          const int32_t *y_a, const int32_t *y_b,
                                          int32_t *u_a, int32_t *u_b, void *stream);
int tfhe_amd_bootstrap_acc_batch_dev(TfheAmdContext *ctx, int B, int n_acc, const int32_t *acc,
                                     const int32_t *acc_index, int32_t c, int32_t sa,
                                     const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                     const int32_t *y_a, const int32_t *y_b,
                                     int32_t *res_a, int32_t *res_b, void *stream);
int tfhe_amd_bootstrap_acc_woks_batch_host(TfheAmdContext *ctx, int B, int n_acc, const int32_t *acc,
                                           const int32_t *acc_index, int32_t c, int32_t sa,
                                           const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                           const int32_t *y_a, const int32_t *y_b,
                                           int32_t *u_a, int32_t *u_b);
int tfhe_amd_bootstrap_acc_batch_host(TfheAmdContext *ctx, int B, int n_acc, const int32_t *acc,
                                      const int32_t *acc_index, int32_t c, int32_t sa,
                                      const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                      const int32_t *y_a, const int32_t *y_b,
                                      int32_t *res_a, int32_t *res_b);

/* The composed p-way selector, p a power of two in [2, 1024].  cand_a [p][B][500], cand_b [p][B] are
 * the candidates, function-major: exactly what tfhe_amd_bootstrap_lut_many_batch_* or p LUT batches
 * write.  Query q's selector is (0, c) + sa*Y_q.  Four steps: the pack of B outputs of p inputs with
 * candidate m at coefficient m (1024 / p), into the pack key's accumulator scratch (8 KB per query,
 * beside its digit scratch, grown and fenced across streams the same way); the box fill with
 * log_w = 10 - log2 p; the rotation of accumulator q by selector q; the key switch.  res_q has the
 * phase of cand[m_q][q] plus noise, m_q the box of the selector's phase among the p boxes of [0, 1/2);
 * a selector phase in [1/2, 1) gives the negated candidate.  A gate bit (+-1/8) selects with p = 2,
 * c = 1/4, sa = 1.  With bootstrapped candidates and a bootstrapped selector p <= 4 decodes with
 * margin.  res may alias Y or the candidates.  TFHE_AMD_E_ARG for a p that is no
 * such power of two, B < 0, null arrays, a null key or context, a key on another device and a context
 * without bootstrapping or key-switching key; B = 0 returns TFHE_AMD_OK.  tfhe_amd_last_kernels lists
 * "k_pack_digits(function-major)", the pack kernel, "k_tlwe_box_fill", the tlwe rotation and the key
 * switch in order. */
int tfhe_amd_select_batch_dev(TfheAmdContext *ctx, TfheAmdPackKey *pack_key, int B, int p,
                              const int32_t *cand_a, const int32_t *cand_b, int32_t c, int32_t sa,
                              const int32_t *y_a, const int32_t *y_b, int32_t *res_a, int32_t *res_b,
                              void *stream);
int tfhe_amd_select_batch_host(TfheAmdContext *ctx, TfheAmdPackKey *pack_key, int B, int p,
                               const int32_t *cand_a, const int32_t *cand_b, int32_t c, int32_t sa,
                               const int32_t *y_a, const int32_t *y_b, int32_t *res_a, int32_t *res_b);

/* Timing of the engine's own kernels (HIP events on the stream they run on):
 * enable=1 starts accumulating; read returns the summed ms and launch counts of the
 * blind-rotation kernel and the key-switch kernel since enabling. */
int tfhe_amd_profile_enable(TfheAmdContext *ctx, int enable);
int tfhe_amd_profile_read(TfheAmdContext *ctx, double *br_ms, int *br_launches,
                          double *ks_ms, int *ks_launches);

/* ---------------------------------------------------------------- several GPUs
 * A multi-device context holds one replica of the key per device (uploaded and converted on
 * each device concurrently) and one worker thread per device.  A batch of independent gates
 * is split into contiguous shards whose sizes differ by at most one (tfhe_amd_shard_range,
 * the arithmetic of cpu-gpu-tfhe_amd/shard.py); every device runs its shard through the
 * single-device host path and writes disjoint rows of the caller's arrays.  No collective.
 * Generalizes the reference's per-batch chunk loop (gpuParallel/boot-gates.cu:2869-2907) from
 * one GPU to all of them.  `devices` may repeat a device (several contexts on one GPU). */
typedef struct TfheAmdMulti TfheAmdMulti;
int tfhe_amd_multi_create(const TFheGateBootstrappingCloudKeySet *bk, int device_mask, TfheAmdMulti **out);
int tfhe_amd_multi_create_raw(const int32_t *bk, const int32_t *ksk, const int *devices, int ndev,
                              TfheAmdMulti **out);
int tfhe_amd_multi_destroy(TfheAmdMulti *m);
/* the device list (returns its length; fills up to cap entries) */
int tfhe_amd_multi_devices(const TfheAmdMulti *m, int *devices, int cap);
/* the context of device slot i (profiling, guard statistics); owned by the multi-context */
TfheAmdContext *tfhe_amd_multi_context(TfheAmdMulti *m, int i);
/* B gates over the devices, host SoA arrays as tfhe_amd_gate_batch_host; synchronous */
int tfhe_amd_multi_gate_batch_host(TfheAmdMulti *m, int gate, int B, int32_t *res_a, int32_t *res_b,
                                   const int32_t *ca_a, const int32_t *ca_b, const int32_t *cb_a,
                                   const int32_t *cb_b, const int32_t *cc_a, const int32_t *cc_b);
/* Device-resident shards (no PCIe in the loop): slot i's shard of counts[i] gates lives on slot
 * i's device (arrays of per-slot device pointers, SoA as tfhe_amd_gate_batch_dev; cc_* for MUX
 * only, may be NULL otherwise); enqueued on streams[i] (NULL array or entry = the slot context's
 * own stream) and returns without waiting. */
int tfhe_amd_multi_gate_batch_dev(TfheAmdMulti *m, int gate, const int *counts, int32_t *const *res_a,
                                  int32_t *const *res_b, const int32_t *const *ca_a, const int32_t *const *ca_b,
                                  const int32_t *const *cb_a, const int32_t *const *cb_b,
                                  const int32_t *const *cc_a, const int32_t *const *cc_b, void *const *streams);
/* waits for the own stream of every slot context */
int tfhe_amd_multi_sync(TfheAmdMulti *m);
/* A circuit (below) over the devices, device-resident: slot i evaluates counts[i] instances in its
 * own wire arrays [n_wires][counts[i]][500] / [n_wires][counts[i]] (input wires filled); enqueued,
 * returns without waiting. */
int tfhe_amd_multi_circuit_run_dev(TfheAmdMulti *m, TfheAmdCircuit *circ, const int *counts,
                                   int32_t *const *wires_a, int32_t *const *wires_b, void *const *streams);
/* The same from host memory, synchronous: B instances in contiguous shards (tfhe_amd_shard_range);
 * in_a [n_in][B][500], in_b [n_in][B] hold the input wires in_wires[k]; each device copies in its
 * shard, evaluates in its own HBM and copies its shard of the wires out_wires[k] back into
 * out_a [n_out][B][500], out_b [n_out][B].  The reference's matrix-vector product
 * (BOOTS_matrixMultiplication, gpuParallel/main.cu:2342-2462) over every GPU of a node. */
int tfhe_amd_multi_circuit_run_host(TfheAmdMulti *m, TfheAmdCircuit *circ, int B, int n_in, const int *in_wires,
                                    const int32_t *in_a, const int32_t *in_b, int n_out, const int *out_wires,
                                    int32_t *out_a, int32_t *out_b);
/* shard [lo, hi) of `total` gates for rank of world */
int tfhe_amd_shard_range(long long total, int rank, int world, long long *lo, long long *hi);

/* SURVEY.md §8(b) Tier-2 names: tfhe_gpu_init builds (or replaces) the multi-device context of
 * a cloud key over device_mask (bit d = GPU d); tfhe_gpu_boots_batch runs B gates of one kind
 * (TFHE_GATE_*; c_* for MUX only) over it, or over the key's Tier-1 device when no multi-device
 * context was registered.  The context is dropped with the key. */
int tfhe_gpu_init(const TFheGateBootstrappingCloudKeySet *bk, int device_mask);
int tfhe_gpu_boots_batch(int gate, int32_t *res_a, int32_t *res_b, const int32_t *a_a, const int32_t *a_b,
                         const int32_t *b_a, const int32_t *b_b, const int32_t *c_a, const int32_t *c_b, int B,
                         const TFheGateBootstrappingCloudKeySet *bk);

/* Convenience: the same batch over LweSample arrays (Tier-1 structs) with the device
 * context cached per cloud key.  Each sample's a row is gathered straight into pinned staging and
 * each result scattered straight back (slices of 1 024 pipelined); result may be the same array as
 * an input; current_variance is set as the reference's lweKeySwitch sets it (summed on the GPU in
 * the reference's order).  Returns TFHE_AMD_OK or an error code (c may be NULL unless gate = MUX). */
int tfhe_amd_boots_batch(int gate, LweSample *result, const LweSample *a, const LweSample *b,
                         const LweSample *c, int B, const TFheGateBootstrappingCloudKeySet *bk);

/* Number of per-thread lanes (stream + scratch) the Tier-1 API holds for this cloud key;
 * a thread's lanes are released when it exits (0 if the key has no device context). */
int tfhe_amd_tier1_lane_count(const TFheGateBootstrappingCloudKeySet *bk);

/* Concurrent Tier-1 gate calls on one key are coalesced: a calling thread enqueues its gate; a
 * waiting thread that finds one of the queue's two lanes free becomes the leader of the next
 * batch: it waits until every thread inside a gate call and not in a running batch has enqueued
 * (an adaptive window: 200 us at first, then 4x the observed wait + 20 us, within 200 - 1000 us),
 * takes every pending gate and runs them on its lane — one gate kind
 * as one gate batch, several kinds as one mixed launch (one blind rotation + one key switch) per
 * 512 gates — while later calls queue for the next batch, which the other lane can stage and
 * launch while this one is still running (a lone thread runs its gate at once, B = 1).  Results,
 * aliasing and current_variance are as for a lone call.  env TFHE_AMD_TIER1_COALESCE=0 disables
 * the queue (per-thread lanes, B = 1 launches).
 * queue_stats: batches run, gates they held, the largest batch (reset = 1 zeroes them). */
int tfhe_amd_tier1_queue_stats(const TFheGateBootstrappingCloudKeySet *bk, long long *batches, long long *gates,
                               long long *largest, int reset);
/* Where the queue's time went, in ms summed over its batches since the last reset: ms[0] the
 * leaders' straggler waits, [1] packing the requests, [2] the device gate batches (staging, copies,
 * kernels incl. the current_variance sums of single-kind batches, synchronize), [3] the device
 * current_variance sums of mixed-kind batches, [4] unpacking, [5] 0 (reserved). */
int tfhe_amd_tier1_queue_times(const TFheGateBootstrappingCloudKeySet *bk, double ms[6], int reset);
/* Build the key's Tier-1 device context now (HIP initialisation, key upload and conversion on the
 * device, the queue's stream and scratch: 0.1-0.3 s once per process and key) instead of inside
 * the first gate call. */
int tfhe_amd_tier1_prepare(const TFheGateBootstrappingCloudKeySet *bk);

/* Device selection for the Tier-1 (single-gate) API: the GPU used by the cached
 * context of every cloud key (default 0). */
int tfhe_amd_set_default_device(int device);

/* Key material export (host): bk int32 [500][4][2][1024], ksk int32 [1024][8][4][501] */
int tfhe_amd_export_bk(const TFheGateBootstrappingCloudKeySet *bk, int32_t *out);
int tfhe_amd_export_ksk(const TFheGateBootstrappingCloudKeySet *bk, int32_t *out);
/* LWE secret key (int32 [500]) of a secret keyset */
int tfhe_amd_export_lwe_key(const TFheGateBootstrappingSecretKeySet *key, int32_t *out);
/* TLWE secret key (int32 [1024]; k = 1), = the extracted LWE key of woKS outputs */
int tfhe_amd_export_tlwe_key(const TFheGateBootstrappingSecretKeySet *key, int32_t *out);

/* Select the blind-rotation kernel generation: 0 = default (= 6: fp64 FFT external product,
 * the reference's arithmetic, with the exactness guard above), 4 = the exact 2-prime NTT kernel for
 * every launch.  Returns
 * TFHE_AMD_E_ARG for a generation this build lacks.  Process-wide; results are identical. */
int tfhe_amd_select_kernel(int br_version);

/* The kernels (with the variant the launch geometry picked, e.g. "k_blind_rotate_v6(reg-rotation)",
 * "k_blind_rotate_v4(guard)", "k_keyswitch_v5(int8-mfma+split2)") that the context's last batch
 * call enqueued, comma-separated in first-launch order, NUL-terminated into buf[cap].  Returns the
 * full length (which may exceed cap - 1).  For smoke / bench reports of which kernels produced
 * the checked outputs. */
int tfhe_amd_last_kernels(TfheAmdContext *ctx, char *buf, int cap);

/* Exactness guard of the default fp64 FFT blind rotation: every launch checks
 * every rounded external-product coefficient of every ciphertext over its 500 steps against
 * |c - rint(c)| < 1/8 (through the rounding shifter's quarter-ulp bits) and |c| < 2^49; a
 * ciphertext that breaks either (or whose sampled distance reaches a lower threshold set below)
 * is recomputed by the exact 2-prime NTT kernel in the same stream before its key switch.  The rule is statistical, not a proof: a
 * wrong coefficient needs an FFT error >= 1/2, and one that shows a distance < 1/8 needs >= 7/8
 * while all ~10^6 other roundings of that ciphertext stay below 1/8 (real keys: largest
 * distance 0.06-0.08, FFT errors of one step spread over all its coefficients).  guard_stats reads (and optionally resets)
 * the context's largest distance over the sampled coefficients (one per lane and CMux step) and
 * its count of recomputed ciphertexts (it synchronizes the device).  set_guard_threshold is
 * process-wide and can only make the guard stricter: 0 <= distance <= 1/8 (0 recomputes
 * everything: tests), anything else returns TFHE_AMD_E_ARG.  There is no way to turn the guard
 * off. */
int tfhe_amd_guard_stats(TfheAmdContext *ctx, double *max_distance, long long *recomputed, int reset);
int tfhe_amd_set_guard_threshold(double distance);

/* build tag, e.g. "tfhe_amd gfx950 fft64 br-v6 ks-v4" */
const char *tfhe_amd_version(void);

/* Measurement (not on the bootstrapping path): the fp64 FMA rate the device sustains under its
 * power limit, for the roofline in bench.py.  Every SIMD runs `waves_per_simd` waves of
 * independent register-operand v_fma_f64 chains for about `seconds` (<= 30); *tflops = FLOP/s
 * / 1e12 (FMA = 2), *mhz = the shader clock held meanwhile.  0 on success. */
int tfhe_amd_fp64_ceiling(int device, int waves_per_simd, double seconds, double *tflops, double *mhz);

/* ---------------------------------------------------------------- circuits (§8(f) row 1)
 * A circuit is a DAG of gates over SSA wires (ids 0, 1, ... in creation order; every wire
 * is written once).  tfhe_amd_circuit_run_dev evaluates B independent instances: wires are
 * device arrays a [n_wires][B][500], b [n_wires][B] (wire w of instance k at w*B + k), the
 * input wires filled by the caller.  The compiler levels the DAG by bootstrap depth; each
 * level is ONE blind-rotation launch over all of its gates x B instances and ONE key-switch
 * launch (the reference's compound ANDXOR / XORXOR gates, boot-gates.cu:3027-3098, are the
 * two-gate case).  NOT / COPY / CONST cost no bootstrap: they are folded into the gates that
 * read them (and also written to their own wires).
 * Builders return the new wire id (>= 0) or a negative TFHE_AMD_E* code. */
int tfhe_amd_circuit_create(TfheAmdCircuit **out);
int tfhe_amd_circuit_destroy(TfheAmdCircuit *c);
/* number of contexts the circuit holds device state (level tables, scratch) for; a context's
 * state is dropped when the context is destroyed */
int tfhe_amd_circuit_state_count(TfheAmdCircuit *c);
/* `count` fresh input wires; returns the first id */
int tfhe_amd_circuit_inputs(TfheAmdCircuit *c, int count);
/* one gate (TFHE_GATE_*); unused inputs ignored (MUX: a ? b : cc; CONST: a = bit value) */
int tfhe_amd_circuit_gate(TfheAmdCircuit *c, int gate, int a, int b, int cc);
/* a bootstrapped linear combination: sign((0, c0) + sa*a + sb*b + sc*cc) -> {-1/8, +1/8}
 * (b, cc may be -1); the building block of threshold gates */
int tfhe_amd_circuit_lincomb(TfheAmdCircuit *c, int32_t c0, int32_t sa, int a, int32_t sb, int b, int32_t sc,
                             int cc);
/* Programmable-bootstrap nodes (the batch form and the encoding convention: above, at
 * tfhe_amd_lut_fill).  tfhe_amd_circuit_lut_table registers a copy of a test vector with the
 * circuit and returns its table id (>= 0); tfhe_amd_circuit_lut_table_get reads one back.
 * tfhe_amd_circuit_lut adds one bootstrapped row, levelled like any other:
 * wire = KS(SampleExtract_0(BlindRotate((0, X^{2N - barb} tv[table])))) for the input
 * (0, c0) + sa*a + sb*b + sc*cc (b, cc may be -1).  It may share a level, and so one launch, with
 * gate rows and with rows of other tables; the tables travel to each device with the level
 * tables.  The output is whatever the table holds, so bit gates and the integer builders below
 * may only read it if the table's values are +-1/8.  TFHE_AMD_E_ARG for an unknown table or
 * wire. */
int tfhe_amd_circuit_lut_table(TfheAmdCircuit *c, const int32_t tv[1024]);
int tfhe_amd_circuit_lut(TfheAmdCircuit *c, int table, int32_t c0, int32_t sa, int a, int32_t sb, int b,
                         int32_t sc, int cc);
int tfhe_amd_circuit_lut_table_get(const TfheAmdCircuit *c, int table, int32_t out[1024]);
/* node w as built: kind 0 input / 1 bootstrapped / 2 linear, gate code (-1 = lincomb),
 * constant, coefficients[3], inputs[3] (for host-side plaintext evaluation in tests).
 * A LUT node reports kind 1, gate code -2 and its TABLE ID in *c0 (coefficients and inputs as a
 * lincomb); its constant c0 is read with tfhe_amd_circuit_lut_node, which returns
 * TFHE_AMD_E_ARG for any other node.  The fields of all other node kinds are as before. */
int tfhe_amd_circuit_node(const TfheAmdCircuit *c, int w, int *kind, int *gate, int32_t *c0, int32_t *s, int *in);
int tfhe_amd_circuit_lut_node(const TfheAmdCircuit *c, int w, int *table, int32_t *c0);
/* Many-LUT node (the batch form: tfhe_amd_bootstrap_lut_many_*): ONE bootstrapped row that
 * defines n_out consecutive wires, wire first + f = KS(SampleExtract_f(BlindRotate(...))) with the
 * modulus switch to a multiple of 2^log_nu; returns the first wire id.  It is levelled like any
 * row and may share a level, and so one blind-rotation launch, with gate rows, LUT rows and
 * many-LUT rows of another log_nu; its outputs are n_out entries of the level's one key-switch
 * launch.  tfhe_amd_circuit_info counts one bootstrap and one gate per node and n_out wires,
 * tfhe_amd_circuit_level_sizes one row.  TFHE_AMD_E_ARG (nothing added) for an unknown table or
 * wire, log_nu outside [0, 4] or n_out outside [1, 2^log_nu].
 * tfhe_amd_circuit_node reports each of the node's wires as kind 1, gate code -3, the TABLE ID in
 * *c0 and coefficients and inputs as a lincomb; tfhe_amd_circuit_lut_many_node returns the rest
 * (index = the position of w within its node, the extraction index) and TFHE_AMD_E_ARG for any
 * other node. */
int tfhe_amd_circuit_lut_many(TfheAmdCircuit *c, int table, int log_nu, int n_out, int32_t c0, int32_t sa, int a,
                              int32_t sb, int b, int32_t sc, int cc);
int tfhe_amd_circuit_lut_many_node(const TfheAmdCircuit *c, int w, int *table, int32_t *c0, int *log_nu, int *n_out,
                                   int *index);
/* ---- One-rotation adder cells.  Two encodings of a bit:
 *   TFHE_AMD_ENC_GATE (G): -1/8 for 0, +1/8 for 1: what every gate and every builder above reads
 *     and writes;
 *   TFHE_AMD_ENC_HALF (H): 1/16 for 0, 3/16 for 1, the boxes 0 and 1 of tfhe_amd_lut_fill's
 *     convention at p = 4.
 * Two or three H bits plus -(k - 1)/16 sum to the centre of box m = a + b (+ cin) in [0, 3], which
 * fills the half torus exactly, so ONE many-LUT row (p = 4, log_nu = 1, n_out = 2) returns the sum
 * bit m & 1 (index 0) and the carry m >> 1 (index 1), where a full adder of gate rows takes XOR3
 * and MAJ, two blind rotations.  Each of the two outputs is emitted in H or in G independently:
 * four tables, tfhe_amd_full_add_table(tv, enc_sum, enc_carry) =
 * tfhe_amd_lut_fill_many(tv, 4, 1, 2, {enc_sum(m & 1), enc_carry(m >> 1)}); host only, needs no
 * GPU, TFHE_AMD_E_ARG for an unknown encoding or a null tv.  The cell decodes while the summed
 * phase error of its inputs stays below 1/16 (measured 7 sigma with three
 * bootstrapped inputs; the gate rows have 15).  Digits wider than one bit do NOT survive
 * bootstrapped inputs on this parameter set (ibid.), so there are no radix-4 builders.
 *
 * THE LIBRARY CANNOT CHECK AN ENCODING: a wire is a ciphertext.  Handing a G wire to an entry that
 * reads H (full_add, add_half, to_gate) or an H wire to one that reads G (every gate, every other
 * builder, to_half, and_half) gives a wrong result, not an error.
 *
 * tfhe_amd_circuit_affine: the bootstrap-free node W = (0, c0) + s * W[a] for any c0 and s.  Like
 * NOT / COPY / CONST it is folded into the rows that read it and also written to its own wire;
 * tfhe_amd_circuit_node reports kind 2, gate code -4, c0, s in coefficients[0] and a in inputs[0].
 * The noise of W[a] is multiplied by |s|.
 * tfhe_amd_circuit_to_gate: H -> G, the affine node 2 H - 1/4 (no bootstrap; the noise doubles).
 * tfhe_amd_circuit_to_half: G -> H, one bootstrap: a sign row through the constant test vector
 *   1/16, then the affine node + 1/8; returns the affine node's wire (two wires are added).
 * tfhe_amd_circuit_and_half: the AND of two G bits as an H bit, one bootstrap: the sign row
 *   -1/8 + a + b through the constant test vector 1/16, then + 1/8 (two wires are added).
 * tfhe_amd_circuit_full_add: one many-LUT node on the H wires a, b and cin (cin = -1: a half
 *   adder); *sum and *carry receive the wires, emitted in enc_sum and enc_carry.  carry = NULL
 *   makes an n_out = 1 row (a carry that is dropped).  The tables are registered with the circuit
 *   at first use and shared by all its cells: a circuit holds at most four of them and the one
 *   constant test vector.  Returns 0, or TFHE_AMD_E_ARG with nothing added for an unknown wire or
 *   encoding (both encodings are checked even when carry is NULL) or a null sum.
 * All return the new wire (affine, to_gate, to_half, and_half) or a negative TFHE_AMD_E* code. */
enum { TFHE_AMD_ENC_GATE = 0, TFHE_AMD_ENC_HALF = 1 };
int tfhe_amd_full_add_table(int32_t tv[1024], int enc_sum, int enc_carry);
int tfhe_amd_circuit_affine(TfheAmdCircuit *c, int32_t c0, int32_t s, int a);
int tfhe_amd_circuit_to_gate(TfheAmdCircuit *c, int a);
int tfhe_amd_circuit_to_half(TfheAmdCircuit *c, int a);
int tfhe_amd_circuit_and_half(TfheAmdCircuit *c, int a, int b);
int tfhe_amd_circuit_full_add(TfheAmdCircuit *c, int a, int b, int cin, int enc_sum, int enc_carry, int *sum,
                              int *carry);
/* The builders on these cells.  mul_fa / dot_fa take and return G bits and the arguments of
 * tfhe_amd_circuit_mul / _dot: the partial products leave their AND row as H bits (and_half, one
 * bootstrap each as before), every full and half adder of the same Dadda schedule is one full_add
 * row, and the last two rows go through to_gate into tfhe_amd_circuit_add_prefix (missing bits
 * stay the G constant 0).  Same depth as mul / dot, one bootstrap less per adder cell.
 * add_half: ripple add of two vectors of H bits (carry_in an H bit or -1), one row per bit where
 * tfhe_amd_circuit_add has two; the sum bits and the returned carry-out wire are emitted in
 * enc_out, so a chain of additions can stay in H.  TFHE_AMD_E_ARG for an unknown wire or encoding,
 * nbits <= 0 or a null array. */
int tfhe_amd_circuit_mul_fa(TfheAmdCircuit *c, int nbits, const int *a, const int *b, int *prod);
int tfhe_amd_circuit_dot_fa(TfheAmdCircuit *c, int nterms, int nbits, const int *a, const int *b, int out_bits,
                            int *out);
int tfhe_amd_circuit_add_half(TfheAmdCircuit *c, int nbits, const int *a, const int *b, int carry_in, int enc_out,
                              int *sum);
/* compile (if needed) and report size: wires, gates, bootstraps per instance, depth */
int tfhe_amd_circuit_info(TfheAmdCircuit *c, int *n_wires, int *n_gates, int *n_bootstraps, int *depth);
/* rows (bootstraps) per level, level 0 first (level 0 is bootstrap-free); returns #levels */
int tfhe_amd_circuit_level_sizes(TfheAmdCircuit *c, int *rows_per_level, int cap);
int tfhe_amd_circuit_run_dev(TfheAmdContext *ctx, TfheAmdCircuit *c, int B, int32_t *wires_a, int32_t *wires_b,
                             void *stream);
/* ---- Select nodes (the batch form: tfhe_amd_select_batch_*).  A computed digit picks
 * among computed wires inside the DAG.  tfhe_amd_circuit_select adds one node on p in {2, 4, 8, 16}
 * candidate wires cand[0 .. p) and the selector (0, c0) + s * W[sel]; it returns the output wire.
 * Semantics are those of tfhe_amd_select_batch_*: the box of the selector's phase among the p boxes
 * of [0, 1/2) picks the candidate, a phase in [1/2, 1) gives the NEGATED candidate; a gate bit
 * selects with p = 2, c0 = 1/4, s = 1.  The candidates are read as written to their wires (any value,
 * any node kind, inputs and CONST included), the selector folds through NOT / COPY / affine chains
 * like any row input.  The node sits one level above the deepest of the selector's base and the
 * candidates, counts one bootstrap (tfhe_amd_circuit_info) and one row
 * (tfhe_amd_circuit_level_sizes), and shares its level's one key-switch launch; the select rows of
 * a level run as a pack, a box fill per distinct p and one rows launch of the blind rotation of
 * their own, after the level's other rows.  TFHE_AMD_E_ARG (nothing added) for another p, a null
 * cand or any wire not yet defined.
 * tfhe_amd_circuit_node reports kind 1, gate code -5, the selector's c0, s in coefficients[0] and
 * sel in inputs[0]; tfhe_amd_circuit_select_node returns p, the candidates (cand[16], -1 beyond p)
 * and c0, and TFHE_AMD_E_ARG for any other node.  tfhe_amd_circuit_select_count: the number of
 * select nodes.
 * tfhe_amd_circuit_lut2: a function of two 2-bit digits x, y (p = 4 boxes of tfhe_amd_lut_fill's
 * convention) in two rotations: one many-LUT node on x with (log_nu, n_out) = (2, 4) whose output j
 * is m -> values[4 j + m] (tfhe_amd_lut_fill_many(tv, 4, 2, 4, values)), then a select node over its
 * four wires driven by y.  Returns the wire of values[4 y + x] (five wires are added).
 * A circuit with a select node needs a packing key at run time: tfhe_amd_circuit_run_pk_dev is
 * tfhe_amd_circuit_run_dev with the key, whose digit and accumulator scratch the select rows use
 * (shared with, and ordered against, every other call on the key).  TFHE_AMD_E_ARG for a null key, a
 * key on another device and a context without bootstrapping or key-switching key.
 * tfhe_amd_circuit_run_dev and both tfhe_amd_multi_circuit_run_* forms return TFHE_AMD_E_ARG for a
 * circuit that holds a select node, before anything is launched (packing keys have no replicas);
 * a circuit without one behaves the same through either run form. */
int tfhe_amd_circuit_select(TfheAmdCircuit *c, int p, const int *cand, int32_t c0, int32_t s, int sel);
int tfhe_amd_circuit_select_node(const TfheAmdCircuit *c, int w, int *p, int cand[16], int32_t *c0);
int tfhe_amd_circuit_select_count(const TfheAmdCircuit *c);
int tfhe_amd_circuit_lut2(TfheAmdCircuit *c, const int32_t values[16], int x, int y);
int tfhe_amd_circuit_run_pk_dev(TfheAmdContext *ctx, TfheAmdPackKey *pack_key, TfheAmdCircuit *c, int B,
                                int32_t *wires_a, int32_t *wires_b, void *stream);
/* integer builders over little-endian bit vectors of wire ids (Cipher.cpp's layout):
 * ripple-carry add (XOR3 / MAJ full adders, depth nbits; carry_in may be -1) -> carry wire;
 * subtract a - b -> carry wire; parallel-prefix add (depth 2 + log2 nbits) -> carry wire;
 * unsigned multiply nbits x nbits -> 2 nbits (AND partial products, carry-save tree,
 * prefix adder) */
int tfhe_amd_circuit_add(TfheAmdCircuit *c, int nbits, const int *a, const int *b, int carry_in, int *sum);
int tfhe_amd_circuit_sub(TfheAmdCircuit *c, int nbits, const int *a, const int *b, int *diff);
int tfhe_amd_circuit_add_prefix(TfheAmdCircuit *c, int nbits, const int *a, const int *b, int *sum);
int tfhe_amd_circuit_mul(TfheAmdCircuit *c, int nbits, const int *a, const int *b, int *prod);
/* sum_t a_t * b_t over nterms pairs of nbits-bit operands (a, b: nterms * nbits wires, term
 * major) into out_bits bits, mod 2^out_bits: one Dadda tree over all partial products */
int tfhe_amd_circuit_dot(TfheAmdCircuit *c, int nterms, int nbits, const int *a, const int *b, int out_bits,
                         int *out);

/* Cipher's remaining operators (cpuParallel/Cipher.cpp) as level-batched circuits:
 * compare: op 0 a > b, 1 a >= b, 2 a < b, 3 a <= b, 4 a == b, 5 a != b (two's complement when
 *   is_signed; operator> / <= / ==, :597-644) -> the result wire (log-depth trees);
 * minmax: min (want_max = 0, minimum :314-333) or max, one comparison + one MUX level;
 * neg: two's complement (twosComplement :300-311); abs: |a| (absolute :483-505);
 * divu: unsigned restoring division, q = a / b, r = a % b (r nullable; b = 0: q all ones, r = a);
 * div: signed division truncated toward zero (operator/, divInternal, addSign :507-589).
 * All return 0 (or the wire id for compare) or a negative TFHE_AMD_E* code. */
enum { TFHE_AMD_CMP_GT = 0, TFHE_AMD_CMP_GE = 1, TFHE_AMD_CMP_LT = 2, TFHE_AMD_CMP_LE = 3,
       TFHE_AMD_CMP_EQ = 4, TFHE_AMD_CMP_NE = 5 };
int tfhe_amd_circuit_compare(TfheAmdCircuit *c, int nbits, const int *a, const int *b, int op, int is_signed);
int tfhe_amd_circuit_minmax(TfheAmdCircuit *c, int nbits, const int *a, const int *b, int want_max, int is_signed,
                            int *out);
int tfhe_amd_circuit_neg(TfheAmdCircuit *c, int nbits, const int *a, int *out);
int tfhe_amd_circuit_abs(TfheAmdCircuit *c, int nbits, const int *a, int *out);
int tfhe_amd_circuit_divu(TfheAmdCircuit *c, int nbits, const int *a, const int *b, int *q, int *r);
int tfhe_amd_circuit_div(TfheAmdCircuit *c, int nbits, const int *a, const int *b, int *q);

/* ---- Key ring: mixed-key batches.  A context is one cloud key and every batch
 * entry point above takes one context; a ring names 1 .. 256 contexts of ONE device as its slots
 * 0 .. n_keys - 1, and its batch entry points take ciphertexts of any of those keys in one call:
 * ciphertext b belongs to slot key_of[b], in any order, and all of them share one blind-rotation
 * launch chain (each row under its own bootstrapping key) and one guard launch; the key switch runs
 * once per slot that has ciphertexts in the call.  Results are, word for word, what each member's
 * own entry points give on its ciphertexts.
 * The ring BORROWS its members' device keys: it neither copies nor frees them, and it owns only a
 * small device table of per-slot key pointers and its row tables.  LIFETIME: destroy the ring before
 * any of its members.  The same context may sit in several slots.
 * A ring call executes in member 0's frame: its stream when `stream` is NULL, its scratch, its guard
 * counters and its launch trace, so tfhe_amd_guard_stats, tfhe_amd_last_kernels and tfhe_amd_sync
 * on member 0 report ring calls.  Calls on one ring are serialised.
 * Anything but 1 <= n_keys <= 256 contexts on one device, each with a bootstrapping and a
 * key-switching key, is TFHE_AMD_E_ARG. */
typedef struct TfheAmdKeyRing TfheAmdKeyRing;
int tfhe_amd_keyring_create(TfheAmdContext *const *ctxs, int n_keys, TfheAmdKeyRing **out);
int tfhe_amd_keyring_destroy(TfheAmdKeyRing *ring);
int tfhe_amd_keyring_count(const TfheAmdKeyRing *ring);    /* slots, or TFHE_AMD_E_ARG */
int tfhe_amd_keyring_device(const TfheAmdKeyRing *ring);   /* device index, or -1 */
/* The order a ring call works in (pure host function): order [B] = the batch indices sorted by key
 * slot, stable; offsets [n_keys + 1] = where each slot's group starts in `order`; *rows = the blind
 * rotations of the batch (a MUX counts two, TFHE_GATE_NOT / TFHE_GATE_COPY none; gates == NULL: one
 * per ciphertext, the LUT form).  Any output may be NULL.  TFHE_AMD_E_ARG for B < 0, n_keys outside
 * [1, 256], a slot outside [0, n_keys) or a gate the ring's gate forms do not take. */
int tfhe_amd_keyring_plan(int B, int n_keys, const int *key_of, const int *gates,
                          int *order, int *offsets, int *rows);
/* B gates of mixed kinds over mixed keys: gates [B] and key_of [B] are HOST arrays (as gates is in
 * tfhe_amd_gate_batch_mixed_host); gate kinds TFHE_GATE_NAND .. TFHE_GATE_MUX as there, and the
 * linear TFHE_GATE_NOT / TFHE_GATE_COPY of ca (no bootstrap, no key).  cb_* may be NULL when every
 * gate is linear, cc_* when none is a MUX.  A bad slot or gate code is TFHE_AMD_E_ARG before anything
 * is launched or written; B = 0 is TFHE_AMD_OK with no launch.  The inputs are read in place and
 * res [0, B) is all that is written; res may alias an input array (entry for entry). */
int tfhe_amd_keyring_gate_batch_dev(TfheAmdKeyRing *ring, int B, const int *gates, const int *key_of,
                                    int32_t *res_a, int32_t *res_b,
                                    const int32_t *ca_a, const int32_t *ca_b,
                                    const int32_t *cb_a, const int32_t *cb_b,
                                    const int32_t *cc_a, const int32_t *cc_b, void *stream);
int tfhe_amd_keyring_gate_batch_host(TfheAmdKeyRing *ring, int B, const int *gates, const int *key_of,
                                     int32_t *res_a, int32_t *res_b,
                                     const int32_t *ca_a, const int32_t *ca_b,
                                     const int32_t *cb_a, const int32_t *cb_b,
                                     const int32_t *cc_a, const int32_t *cc_b);
/* Programmable bootstrap + key switch of x over mixed keys (tfhe_amd_bootstrap_lut_batch_* with
 * cst = 0, sa = 1, sb = 0): tv [n_lut][1024] and lut_index [B] (NULL: table 0; clamped by the kernel)
 * are device arrays in the dev form and host arrays in the host form; key_of is a host array. */
int tfhe_amd_keyring_bootstrap_lut_batch_dev(TfheAmdKeyRing *ring, int B, const int *key_of, int n_lut,
                                             const int32_t *tv, const int32_t *lut_index,
                                             int32_t *res_a, int32_t *res_b,
                                             const int32_t *x_a, const int32_t *x_b, void *stream);
int tfhe_amd_keyring_bootstrap_lut_batch_host(TfheAmdKeyRing *ring, int B, const int *key_of, int n_lut,
                                              const int32_t *tv, const int32_t *lut_index,
                                              int32_t *res_a, int32_t *res_b,
                                              const int32_t *x_a, const int32_t *x_b);

/* ---- Mixed-key circuits.  One run of a circuit over B instances, instance k under
 * the cloud key of ring slot key_of[k] (HOST array, any order).  Every level takes one blind-rotation
 * launch chain and one guard launch over all rows x instances, each instance under its own
 * bootstrapping key, one key-switch launch over all key groups (one launch per non-empty group when
 * a member lacks the int8 key layout, TFHE_AMD_KS5=0, or the instances are of one slot), and the
 * key-independent linear launch.  Every word of every wire equals what tfhe_amd_circuit_run_dev on
 * the slot's own context writes for that slot's instances.  The run executes in member 0's frame like
 * every ring call; the circuit keeps its level tables and scratch for the ring until the ring is
 * destroyed or the circuit recompiled.
 * wires_a [n_wires][B][500], wires_b [n_wires][B] on the ring's device, input wires filled; enqueued
 * on `stream` (NULL: member 0's), returns without waiting.  TFHE_AMD_E_ARG, before anything is
 * launched or written, for a NULL ring, circuit or key_of, B < 0, a slot outside the ring, NULL wire
 * arrays with B > 0, and a circuit that holds a select node (packing keys are per key); B = 0 is
 * TFHE_AMD_OK with no launch. */
int tfhe_amd_keyring_circuit_run_dev(TfheAmdKeyRing *ring, TfheAmdCircuit *circ, int B, const int *key_of,
                                     int32_t *wires_a, int32_t *wires_b, void *stream);
/* The same from host memory, synchronous, in the shape of tfhe_amd_multi_circuit_run_host: in_a
 * [n_in][B][500], in_b [n_in][B] hold the input wires in_wires[k]; the wires out_wires[k] come back
 * in out_a [n_out][B][500], out_b [n_out][B]. */
int tfhe_amd_keyring_circuit_run_host(TfheAmdKeyRing *ring, TfheAmdCircuit *circ, int B, const int *key_of,
                                      int n_in, const int *in_wires, const int32_t *in_a, const int32_t *in_b,
                                      int n_out, const int *out_wires, int32_t *out_a, int32_t *out_b);
/* The order and the key-switch tiles of such a run (pure host function).  order [B] = the instances
 * sorted by slot, stable; offsets [n_keys + 1] = where each slot's group starts in `order`.  A level
 * with nks key-switched outputs has the lanes nks offsets[g] + o n_g + j of group g (n_g instances):
 * output o at the group's j-th instance.  They are cut into tiles of `tile` lanes that never span two
 * groups; tile t is tiles[3 t .. 3 t + 2] = its slot, its first lane, its live lanes (1 .. tile).
 * *n_tiles = their number; tiles == NULL counts only, else more than tile_cap tiles is TFHE_AMD_E_ARG.
 * Any output may be NULL.  TFHE_AMD_E_ARG also for B < 0, n_keys outside [1, 256], nks < 0, tile < 1,
 * a slot outside [0, n_keys) and nks B above 2^30 - 1.  tfhe_amd_keyring_circuit_tile: the tile size
 * the engine's key switch uses. */
int tfhe_amd_keyring_circuit_plan(int B, int n_keys, const int *key_of, int nks, int tile,
                                  int *order, int *offsets, int *tiles, int tile_cap, int *n_tiles);
int tfhe_amd_keyring_circuit_tile(void);

#ifdef __cplusplus
}
#endif
#endif
