// tfhe_api.cpp — the host-only half of the TFHE C API (Tier-1).
//
// The drop-in boundary of SURVEY.md §8(b), client side: the key / ciphertext lifecycle, key
// generation, encryption and the linear LWE helpers that cpuParallel/Cipher.cpp and cloud.cpp
// call from libtfhe, plus the tfhe_amd_export_* flatteners.  Structs are allocated with the
// reference's layouts (include/tfhe/tfhe.h).  The code restates the reference's CPU code and
// keeps its RNG: std::default_random_engine seeded by tfhe_random_generator_setSeed
// (numeric-functions.cu:11-19), drawn in the reference's order.  Nothing here touches a device:
// the bootstrapped operations (bootsXXX, tfhe_bootstrap_(woKS_)FFT, lweKeySwitch, the L1 entry
// points) are tier1.cpp, which reaches the keys through the four functions api_internal.h
// declares for it.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <mutex>
#include <random>
#include <vector>

#include "params.h"
#include "../../include/tfhe/tfhe.h"
#include "../../include/tfhe_amd.h"
#include "api_internal.h"

using namespace tfhe_amd;
using namespace tfhe_amd::api;

// ------------------------------------------------------------------ numerics
// numeric-functions.cu:11-77

static std::default_random_engine generator;
static std::uniform_int_distribution<Torus32> uniformTorus32_distrib(INT32_MIN, INT32_MAX);
static std::mutex g_rng_mu;   // the reference RNG is global and not thread safe; we lock it

EXPORT void die_dramatically(const char *message) {
    std::cerr << message << std::endl;
    abort();
}

EXPORT void tfhe_random_generator_setSeed(uint32_t *values, int size) {
    std::lock_guard<std::mutex> lk(g_rng_mu);
    std::seed_seq seeds(values, values + size);
    generator.seed(seeds);
}

EXPORT Torus32 dtot32(double d) { return int32_t(int64_t((d - int64_t(d)) * 4294967296.0)); }
EXPORT double t32tod(Torus32 x) { return double(x) / 4294967296.0; }

static Torus32 gaussian32_nolock(Torus32 message, double sigma) {
    std::normal_distribution<double> distribution(0., sigma);   // fresh per draw, as :24
    double err = distribution(generator);
    return (Torus32)((uint32_t)message + (uint32_t)dtot32(err));
}
EXPORT Torus32 gaussian32(Torus32 message, double sigma) {
    std::lock_guard<std::mutex> lk(g_rng_mu);
    return gaussian32_nolock(message, sigma);
}

EXPORT Torus32 approxPhase(Torus32 phase, int Msize) {
    uint64_t interv = ((UINT64_C(1) << 63) / Msize) * 2;
    uint64_t half_interval = interv / 2;
    uint64_t phase64 = (uint64_t(uint32_t(phase)) << 32) + half_interval;
    phase64 -= phase64 % interv;
    return int32_t(phase64 >> 32);
}
EXPORT int modSwitchFromTorus32(Torus32 phase, int Msize) {
    uint64_t interv = ((UINT64_C(1) << 63) / Msize) * 2;
    uint64_t half_interval = interv / 2;
    uint64_t phase64 = (uint64_t(uint32_t(phase)) << 32) + half_interval;
    return int(phase64 / interv);
}
EXPORT Torus32 modSwitchToTorus32(int mu, int Msize) {
    uint64_t interv = ((UINT64_C(1) << 63) / Msize) * 2;
    uint64_t phase64 = uint64_t(int64_t(mu)) * interv;
    return Torus32(uint32_t(phase64 >> 32));
}

// ------------------------------------------------------------------ params
// tfhe_gate_bootstrapping.cu:25-55; tgsw.cu:7-29; tlwe.cu (extracted params n = k N)
// (ParamsImpl is declared in api_internal.h; alphas are arguments because parameter sets
// read back from a file carry the %.8lf-rounded values, tfhe_generic_streams.cu:37-41)

ParamsImpl::ParamsImpl(double lwe_alpha_min, double lwe_alpha_max, double tlwe_alpha_min, double tlwe_alpha_max)
    : in_out{kn, lwe_alpha_min, lwe_alpha_max},
      accum{kN, kK, tlwe_alpha_min, tlwe_alpha_max, LweParams{kN * kK, tlwe_alpha_min, tlwe_alpha_max}},
      tgsw{kL, kBgbit, 1 << kBgbit, (1 << kBgbit) / 2, (1u << kBgbit) - 1, &accum, kKpl, h, kDecompOffset},
      set{kKsT, kKsBasebit, &in_out, &tgsw} {
    for (int i = 0; i < kL; ++i) h[i] = Torus32(1u << (32 - (i + 1) * kBgbit));
}

static std::mutex g_params_mu;
static std::map<const TFheGateBootstrappingParameterSet *, ParamsImpl *> g_params;

TFheGateBootstrappingParameterSet *tfhe_amd::api::register_params(ParamsImpl *p) {
    std::lock_guard<std::mutex> lk(g_params_mu);
    g_params[&p->set] = p;
    return &p->set;
}

const ParamsImpl *tfhe_amd::api::params_of(const TFheGateBootstrappingParameterSet *params) {
    std::lock_guard<std::mutex> lk(g_params_mu);
    auto it = g_params.find(params);
    if (it == g_params.end()) die_dramatically("tfhe_amd: unknown parameter set");
    return it->second;
}

EXPORT TFheGateBootstrappingParameterSet *new_default_gate_bootstrapping_parameters(int minimum_lambda) {
    if (minimum_lambda > 128)
        die_dramatically("Sorry, for now, the parameters are only implemented for about 128bit of security!");
    return register_params(new ParamsImpl());
}

EXPORT void delete_gate_bootstrapping_parameters(TFheGateBootstrappingParameterSet *params) {
    std::lock_guard<std::mutex> lk(g_params_mu);
    auto it = g_params.find(params);
    if (it != g_params.end()) {
        delete it->second;
        g_params.erase(it);
    }
}

// ------------------------------------------------------------------ LWE samples
// lwesamples.cu, lwe-functions.cu:21-291

EXPORT LweSample *new_LweSample_array(int nbelts, const LweParams *params) {
    LweSample *s = (LweSample *)malloc(sizeof(LweSample) * (size_t)(nbelts > 0 ? nbelts : 1));
    for (int i = 0; i < nbelts; i++) {
        s[i].a = (Torus32 *)calloc((size_t)params->n, sizeof(Torus32));
        s[i].b = 0;
        s[i].current_variance = 0.;
    }
    return s;
}
EXPORT LweSample *new_LweSample(const LweParams *params) { return new_LweSample_array(1, params); }
EXPORT void delete_LweSample_array(int nbelts, LweSample *obj) {
    if (!obj) return;
    for (int i = 0; i < nbelts; i++) free(obj[i].a);
    free(obj);
}
EXPORT void delete_LweSample(LweSample *obj) { delete_LweSample_array(1, obj); }

EXPORT LweSample *new_gate_bootstrapping_ciphertext(const TFheGateBootstrappingParameterSet *params) {
    return new_LweSample(params->in_out_params);
}
EXPORT LweSample *new_gate_bootstrapping_ciphertext_array(int nbelems, const TFheGateBootstrappingParameterSet *params) {
    return new_LweSample_array(nbelems, params->in_out_params);
}
EXPORT void delete_gate_bootstrapping_ciphertext(LweSample *sample) { delete_LweSample(sample); }
EXPORT void delete_gate_bootstrapping_ciphertext_array(int nbelems, LweSample *samples) {
    delete_LweSample_array(nbelems, samples);
}

LweKey *tfhe_amd::api::new_LweKey(const LweParams *params) {
    LweKey *k = (LweKey *)malloc(sizeof(LweKey));
    *const_cast<const LweParams **>(&k->params) = params;
    k->key = (int *)calloc((size_t)params->n, sizeof(int));
    return k;
}
void tfhe_amd::api::delete_LweKey(LweKey *k) {
    if (!k) return;
    free(k->key);
    free(k);
}

static void lweKeyGen_nolock(LweKey *result) {
    std::uniform_int_distribution<int> distribution(0, 1);
    for (int i = 0; i < result->params->n; i++) result->key[i] = distribution(generator);
}
EXPORT void lweKeyGen(LweKey *result) {
    std::lock_guard<std::mutex> lk(g_rng_mu);
    lweKeyGen_nolock(result);
}

static void lweSymEncrypt_nolock(LweSample *result, Torus32 message, double alpha, const LweKey *key) {
    const int n = key->params->n;
    uint32_t b = (uint32_t)gaussian32_nolock(message, alpha);
    for (int i = 0; i < n; ++i) {
        result->a[i] = uniformTorus32_distrib(generator);
        b += (uint32_t)result->a[i] * (uint32_t)key->key[i];
    }
    result->b = (Torus32)b;
    result->current_variance = alpha * alpha;
}
EXPORT void lweSymEncrypt(LweSample *result, Torus32 message, double alpha, const LweKey *key) {
    std::lock_guard<std::mutex> lk(g_rng_mu);
    lweSymEncrypt_nolock(result, message, alpha, key);
}

static void lweSymEncryptWithExternalNoise_nolock(LweSample *result, Torus32 message, double noise, double alpha,
                                                  const LweKey *key) {
    const int n = key->params->n;
    uint32_t b = (uint32_t)message + (uint32_t)dtot32(noise);
    for (int i = 0; i < n; ++i) {
        result->a[i] = uniformTorus32_distrib(generator);
        b += (uint32_t)result->a[i] * (uint32_t)key->key[i];
    }
    result->b = (Torus32)b;
    result->current_variance = alpha * alpha;
}
EXPORT void lweSymEncryptWithExternalNoise(LweSample *result, Torus32 message, double noise, double alpha,
                                           const LweKey *key) {
    std::lock_guard<std::mutex> lk(g_rng_mu);
    lweSymEncryptWithExternalNoise_nolock(result, message, noise, alpha, key);
}

EXPORT Torus32 lwePhase(const LweSample *sample, const LweKey *key) {
    uint32_t axs = 0;
    for (int i = 0; i < key->params->n; ++i) axs += (uint32_t)sample->a[i] * (uint32_t)key->key[i];
    return (Torus32)((uint32_t)sample->b - axs);
}
EXPORT Torus32 lweSymDecrypt(const LweSample *sample, const LweKey *key, const int Msize) {
    return approxPhase(lwePhase(sample, key), Msize);
}

EXPORT void lweClear(LweSample *r, const LweParams *params) {
    for (int i = 0; i < params->n; ++i) r->a[i] = 0;
    r->b = 0;
    r->current_variance = 0.;
}
EXPORT void lweCopy(LweSample *r, const LweSample *s, const LweParams *params) {
    for (int i = 0; i < params->n; ++i) r->a[i] = s->a[i];
    r->b = s->b;
    r->current_variance = s->current_variance;
}
EXPORT void lweNegate(LweSample *r, const LweSample *s, const LweParams *params) {
    for (int i = 0; i < params->n; ++i) r->a[i] = (Torus32)(0u - (uint32_t)s->a[i]);
    r->b = (Torus32)(0u - (uint32_t)s->b);
    r->current_variance = s->current_variance;
}
EXPORT void lweNoiselessTrivial(LweSample *r, Torus32 mu, const LweParams *params) {
    for (int i = 0; i < params->n; ++i) r->a[i] = 0;
    r->b = mu;
    r->current_variance = 0.;
}
EXPORT void lweAddTo(LweSample *r, const LweSample *s, const LweParams *params) {
    for (int i = 0; i < params->n; ++i) r->a[i] = (Torus32)((uint32_t)r->a[i] + (uint32_t)s->a[i]);
    r->b = (Torus32)((uint32_t)r->b + (uint32_t)s->b);
    r->current_variance += s->current_variance;
}
EXPORT void lweSubTo(LweSample *r, const LweSample *s, const LweParams *params) {
    for (int i = 0; i < params->n; ++i) r->a[i] = (Torus32)((uint32_t)r->a[i] - (uint32_t)s->a[i]);
    r->b = (Torus32)((uint32_t)r->b - (uint32_t)s->b);
    r->current_variance += s->current_variance;
}
EXPORT void lweAddMulTo(LweSample *r, int p, const LweSample *s, const LweParams *params) {
    for (int i = 0; i < params->n; ++i) r->a[i] = (Torus32)((uint32_t)r->a[i] + (uint32_t)p * (uint32_t)s->a[i]);
    r->b = (Torus32)((uint32_t)r->b + (uint32_t)p * (uint32_t)s->b);
    r->current_variance += (p * p) * s->current_variance;
}
EXPORT void lweSubMulTo(LweSample *r, int p, const LweSample *s, const LweParams *params) {
    for (int i = 0; i < params->n; ++i) r->a[i] = (Torus32)((uint32_t)r->a[i] - (uint32_t)p * (uint32_t)s->a[i]);
    r->b = (Torus32)((uint32_t)r->b - (uint32_t)p * (uint32_t)s->b);
    r->current_variance += (p * p) * s->current_variance;
}

// ------------------------------------------------------------------ keys

// Private owners behind the public (reference-layout) structs.  The bootstrapping key is
// kept as one contiguous coefficient-domain block [kn][kpl][k+1][N] — the layout the device
// upload consumes — and the public TGswSample/TLweSample/TorusPolynomial views point into it.
struct BkImpl {
    LweBootstrappingKey pub;
    std::vector<int32_t> coef;                // [kn][4][2][kN]
    std::vector<TorusPolynomial> polys;       // kn*4*2 views
    std::vector<TLweSample> rows;             // kn*4
    std::vector<TLweSample *> blocs;          // kn*(k+1) bloc pointers
    std::vector<TGswSample> gsw;              // kn
    LweKeySwitchKey *ks;
};

struct KskImpl {
    LweKeySwitchKey pub;
    std::vector<int32_t> a;                   // [kN*8*4][kn]
    std::vector<LweSample> samples;           // kN*8*4
    std::vector<LweSample *> l1;              // kN*8
    std::vector<LweSample **> l0;             // kN
};

struct BkFFTImpl {
    LweBootstrappingKeyFFT pub;
    std::vector<int32_t> bk_coef;             // [kn][4][2][kN]   (NTT conversion happens on the GPU)
    LweKeySwitchKey *ks;                      // deep copy (owned)
    // pub.bkFFT: the reference's array of kn TGswSampleFFT (tgsw.h:78-96), so that callers can
    // pass bk->bkFFT + i to tGswFFTExternMulToTLwe; the samples themselves live on the GPU (null
    // all_samples) and an element maps back to (this key, i) through g_gsw (below)
    std::vector<TGswSampleFFT> gsw;
};

// key of every live TGswSampleFFT array: its first element -> the key (L1 entry points)
static std::mutex g_gsw_mu;
static std::map<const TGswSampleFFT *, BkFFTImpl *> g_gsw;
const LweBootstrappingKeyFFT *tfhe_amd::api::gsw_key_of(const TGswSampleFFT *p, int *index) {
    std::lock_guard<std::mutex> lk(g_gsw_mu);
    auto it = g_gsw.upper_bound(p);
    if (it == g_gsw.begin()) return nullptr;
    --it;
    const ptrdiff_t i = p - it->first;
    if (i < 0 || i >= (ptrdiff_t)it->second->gsw.size()) return nullptr;
    *index = (int)i;
    return &it->second->pub;
}

static KskImpl *ksk_of(const LweKeySwitchKey *k) { return reinterpret_cast<KskImpl *>(const_cast<LweKeySwitchKey *>(k)); }
static BkFFTImpl *bkfft_of(const LweBootstrappingKeyFFT *k) {
    return reinterpret_cast<BkFFTImpl *>(const_cast<LweBootstrappingKeyFFT *>(k));
}
const int32_t *tfhe_amd::api::bk_coef_of(const LweBootstrappingKeyFFT *k) { return bkfft_of(k)->bk_coef.data(); }
static BkImpl *bk_of(const LweBootstrappingKey *k) { return reinterpret_cast<BkImpl *>(const_cast<LweBootstrappingKey *>(k)); }

static LweKeySwitchKey *new_ksk(const LweParams *out_params) {
    KskImpl *k = new KskImpl{LweKeySwitchKey{kN, kKsT, kKsBasebit, kKsBase, out_params, nullptr, nullptr, nullptr},
                             {}, {}, {}, {}};
    const size_t ns = (size_t)kN * kKsT * kKsBase;
    k->a.assign(ns * kn, 0);
    k->samples.resize(ns);
    for (size_t s = 0; s < ns; s++) k->samples[s] = LweSample{k->a.data() + s * kn, 0, 0.};
    k->l1.resize((size_t)kN * kKsT);
    for (size_t p = 0; p < k->l1.size(); p++) k->l1[p] = k->samples.data() + kKsBase * p;
    k->l0.resize(kN);
    for (int p = 0; p < kN; p++) k->l0[p] = k->l1.data() + kKsT * p;
    k->pub.ks0_raw = k->samples.data();
    k->pub.ks1_raw = k->l1.data();
    k->pub.ks = k->l0.data();
    return &k->pub;
}
static void delete_ksk(LweKeySwitchKey *k) { delete ksk_of(k); }

// flat [kN][8][4][kn+1] view of any LweKeySwitchKey (ours or foreign-built)
void tfhe_amd::api::ksk_flatten(const LweKeySwitchKey *ks, int32_t *out) {
    for (int i = 0; i < kN; i++)
        for (int j = 0; j < kKsT; j++)
            for (int h = 0; h < kKsBase; h++) {
                const LweSample &s = ks->ks[i][j][h];
                int32_t *dst = out + (((size_t)i * kKsT + j) * kKsBase + h) * (kn + 1);
                memcpy(dst, s.a, sizeof(int32_t) * kn);
                dst[kn] = s.b;
            }
}

LweBootstrappingKey *tfhe_amd::api::new_bk(const ParamsImpl *P) {
    BkImpl *k = new BkImpl{LweBootstrappingKey{&P->in_out, &P->tgsw, &P->accum, &P->accum.extracted_lweparams,
                                               nullptr, nullptr},
                           {}, {}, {}, {}, {}, nullptr};
    k->coef.assign((size_t)kn * kKpl * 2 * kN, 0);
    k->polys.reserve((size_t)kn * kKpl * 2);
    for (size_t p = 0; p < (size_t)kn * kKpl * 2; p++) k->polys.push_back(TorusPolynomial{kN, k->coef.data() + p * kN});
    k->rows.reserve((size_t)kn * kKpl);
    for (size_t r = 0; r < (size_t)kn * kKpl; r++)
        k->rows.push_back(TLweSample{&k->polys[r * 2], &k->polys[r * 2 + 1], 0., kK});
    k->blocs.resize((size_t)kn * (kK + 1));
    for (int i = 0; i < kn; i++)
        for (int b = 0; b <= kK; b++) k->blocs[(size_t)i * (kK + 1) + b] = &k->rows[(size_t)i * kKpl + b * kL];
    k->gsw.reserve(kn);
    for (int i = 0; i < kn; i++)
        k->gsw.push_back(TGswSample{&k->rows[(size_t)i * kKpl], &k->blocs[(size_t)i * (kK + 1)], kK, kL});
    k->ks = new_ksk(&P->in_out);
    k->pub.bk = k->gsw.data();
    k->pub.ks = k->ks;
    return &k->pub;
}
static void delete_bk(LweBootstrappingKey *k) {
    if (!k) return;
    BkImpl *b = bk_of(k);
    delete_ksk(b->ks);
    delete b;
}

// coefficient BK of any LweBootstrappingKey -> flat [kn][4][2][kN]
static void bk_flatten(const LweBootstrappingKey *bk, int32_t *out) {
    for (int i = 0; i < kn; i++)
        for (int p = 0; p < kKpl; p++)
            for (int c = 0; c <= kK; c++)
                memcpy(out + (((size_t)i * kKpl + p) * 2 + c) * kN, bk->bk[i].all_sample[p].a[c].coefsT,
                       sizeof(int32_t) * kN);
}

// new_LweBootstrappingKeyFFT (lwe-bootstrapping-functions-fft.cu:2201 -> :60-89): copy the KSK,
// keep the coefficient BK for the device-side NTT conversion.
LweBootstrappingKeyFFT *tfhe_amd::api::new_bkfft(const LweBootstrappingKey *bk) {
    BkFFTImpl *f = new BkFFTImpl{LweBootstrappingKeyFFT{bk->in_out_params, bk->bk_params, bk->accum_params,
                                                        bk->extract_params, nullptr, nullptr},
                                 {}, nullptr};
    f->bk_coef.resize((size_t)kn * kKpl * 2 * kN);
    bk_flatten(bk, f->bk_coef.data());
    f->ks = new_ksk(bk->in_out_params);
    std::vector<int32_t> flat((size_t)kN * kKsT * kKsBase * (kn + 1));
    ksk_flatten(bk->ks, flat.data());
    KskImpl *dst = ksk_of(f->ks);
    for (size_t s = 0; s < dst->samples.size(); s++) {
        memcpy(dst->samples[s].a, flat.data() + s * (kn + 1), sizeof(int32_t) * kn);
        dst->samples[s].b = flat[s * (kn + 1) + kn];
        dst->samples[s].current_variance = bk->ks->ks0_raw[s].current_variance;
    }
    *const_cast<const LweKeySwitchKey **>(&f->pub.ks) = f->ks;
    f->gsw.reserve(kn);
    for (int i = 0; i < kn; ++i) f->gsw.push_back(TGswSampleFFT{nullptr, nullptr, kK, kL});
    *const_cast<const TGswSampleFFT **>(&f->pub.bkFFT) = f->gsw.data();
    std::lock_guard<std::mutex> lk(g_gsw_mu);
    g_gsw[f->gsw.data()] = f;
    return &f->pub;
}

static void delete_bkfft(LweBootstrappingKeyFFT *k) {
    if (!k) return;
    BkFFTImpl *f = bkfft_of(k);
    {
        std::lock_guard<std::mutex> lk(g_gsw_mu);
        g_gsw.erase(f->gsw.data());
    }
    forget_device_keys(k, f->ks);
    tfhe_amd_internal_forget_multi(k);
    delete_ksk(f->ks);
    delete f;
}

TGswKey *tfhe_amd::api::new_tgsw_key(const ParamsImpl *P) {
    TGswKeyImpl *gk = new TGswKeyImpl{TGswKey{&P->tgsw, &P->accum, nullptr, TLweKey{&P->accum, nullptr}},
                                      std::vector<int>((size_t)kN * kK), IntPolynomial{kN, nullptr}};
    gk->poly.coefs = gk->coefs.data();
    gk->pub.key = &gk->poly;
    gk->pub.tlwe_key.key = &gk->poly;
    return &gk->pub;
}

// lweCreateKeySwitchKey (lwe-keyswitch-functions.cu:890-942)
static void create_ksk_nolock(LweKeySwitchKey *result, const int *in_key /*kN*/, const LweKey *out_key) {
    const int n = result->n, t = result->t, basebit = result->basebit, base = 1 << basebit;
    const double alpha = out_key->params->alpha_min;
    const int sizeks = n * t * (base - 1);
    std::vector<double> noise(sizeks);
    double err = 0;
    for (int i = 0; i < sizeks; ++i) {
        std::normal_distribution<double> distribution(0., alpha);
        noise[i] = distribution(generator);
        err += noise[i];
    }
    err = err / sizeks;
    for (int i = 0; i < sizeks; ++i) noise[i] -= err;
    int index = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < t; ++j) {
            lweNoiselessTrivial(&result->ks[i][j][0], 0, out_key->params);
            for (int h = 1; h < base; ++h) {
                Torus32 mess = (Torus32)((uint32_t)(in_key[i] * h) * (1u << (32 - (j + 1) * basebit)));
                lweSymEncryptWithExternalNoise_nolock(&result->ks[i][j][h], mess, noise[index], alpha, out_key);
                index += 1;
            }
        }
}

// tLweSymEncryptZero (tlwe-functions.cu:26-38) with an EXACT b += key * a (the reference
// uses its FFT multiply here, polynomials_arithmetic.h:112-114; key generation is
// client side and off the hot path)
// on the two polynomials themselves (a, b of kN words): the draws are b's kN Gaussians, then a's
// kN uniform words, which key generation's order below depends on
static void tlwe_zero_rows_nolock(uint32_t *a, uint32_t *b, double alpha, const int *key /*kN binary*/) {
    for (int j = 0; j < kN; ++j) b[j] = (uint32_t)gaussian32_nolock(0, alpha);
    for (int j = 0; j < kN; ++j) a[j] = (uint32_t)uniformTorus32_distrib(generator);   // torusPolynomialUniform
    for (int s = 0; s < kN; ++s) {
        if (!key[s]) continue;           // b += X^s * a (negacyclic)
        for (int i = 0; i < s; ++i) b[i] -= a[i - s + kN];
        for (int i = s; i < kN; ++i) b[i] += a[i - s];
    }
}
static void tlwe_encrypt_zero_nolock(TLweSample *r, double alpha, const int *key /*kN binary*/) {
    tlwe_zero_rows_nolock((uint32_t *)r->a[0].coefsT, (uint32_t *)r->b->coefsT, alpha, key);
    r->current_variance = alpha * alpha;
}

// ---- client side of the leveled mode (include/tfhe_amd.h): TGSW encryptions of
// bits and TLWE encryptions of polynomials under the keyset's TGSW key, in the layout of
// tfhe_amd_export_bk's entries ([4 rows][2: a, b][kN] per sample).  What key generation does inline
// for lwe_key->key[i] above: four zero rows at the key's alpha_min, then tGswAddMuIntH.
EXPORT int tfhe_amd_tgsw_encrypt_bits(const TFheGateBootstrappingSecretKeySet *key, int n, const int32_t *bits,
                                      int32_t *out) {
    if (!key || !key->tgsw_key || n < 0 || !bits || !out) return TFHE_AMD_E_ARG;
    for (int i = 0; i < n; ++i)
        if (bits[i] != 0 && bits[i] != 1) return TFHE_AMD_E_ARG;
    const TGswKey *gk = key->tgsw_key;
    const double alpha = gk->tlwe_params->alpha_min;
    const int *coefs = gk->tlwe_key.key[0].coefs;
    std::lock_guard<std::mutex> lk(g_rng_mu);
    for (int i = 0; i < n; ++i) {
        uint32_t *g = (uint32_t *)out + (size_t)i * kKpl * 2 * kN;
        for (int p = 0; p < kKpl; ++p) tlwe_zero_rows_nolock(g + (size_t)(p * 2) * kN, g + (size_t)(p * 2 + 1) * kN, alpha, coefs);
        for (int bloc = 0; bloc <= kK; ++bloc)
            for (int l = 0; l < kL; l++)
                g[(size_t)((bloc * kL + l) * 2 + bloc) * kN] += (uint32_t)bits[i] * (uint32_t)gk->params->h[l];
    }
    return TFHE_AMD_OK;
}

// mu [n][kN] -> out [n][2: a, b][kN]: a zero row plus the message polynomial on b
EXPORT int tfhe_amd_tlwe_encrypt_polys(const TFheGateBootstrappingSecretKeySet *key, int n, const int32_t *mu,
                                       int32_t *out) {
    if (!key || !key->tgsw_key || n < 0 || !mu || !out) return TFHE_AMD_E_ARG;
    const TGswKey *gk = key->tgsw_key;
    const double alpha = gk->tlwe_params->alpha_min;
    const int *coefs = gk->tlwe_key.key[0].coefs;
    std::lock_guard<std::mutex> lk(g_rng_mu);
    for (int i = 0; i < n; ++i) {
        uint32_t *r = (uint32_t *)out + (size_t)i * 2 * kN;
        tlwe_zero_rows_nolock(r, r + kN, alpha, coefs);
        for (int j = 0; j < kN; ++j) r[kN + j] += (uint32_t)mu[(size_t)i * kN + j];
    }
    return TFHE_AMD_OK;
}

// ---- client side of the packing key switch (include/tfhe_amd.h).  Row (i, j) of the
// key, j = 1 .. kPackT: a zero row under the keyset's TLWE key at its alpha_min (the loop above)
// plus the constant polynomial s_i 2^(32 - 4 j) on b; out [kn][kPackT][2: a, b][kN], rows drawn in
// (i, j) order.
EXPORT int tfhe_amd_pack_key_generate(const TFheGateBootstrappingSecretKeySet *key, int32_t *out) {
    if (!key || !key->tgsw_key || !key->lwe_key || !out) return TFHE_AMD_E_ARG;
    const TGswKey *gk = key->tgsw_key;
    const double alpha = gk->tlwe_params->alpha_min;
    const int *coefs = gk->tlwe_key.key[0].coefs;
    std::lock_guard<std::mutex> lk(g_rng_mu);
    for (int i = 0; i < kn; ++i)
        for (int j = 1; j <= kPackT; ++j) {
            uint32_t *r = (uint32_t *)out + ((size_t)i * kPackT + (j - 1)) * 2 * kN;
            tlwe_zero_rows_nolock(r, r + kN, alpha, coefs);
            r[kN] += (uint32_t)key->lwe_key->key[i] << (32 - kPackBasebit * j);
        }
    return TFHE_AMD_OK;
}

// in [n][2: a, b][kN] -> phase [n][kN] = b - a s mod 2^32 under the keyset's TLWE key (negacyclic)
EXPORT int tfhe_amd_tlwe_phase_polys(const TFheGateBootstrappingSecretKeySet *key, int n, const int32_t *in,
                                     int32_t *phase) {
    if (!key || !key->tgsw_key || n < 0 || !in || !phase) return TFHE_AMD_E_ARG;
    const int *coefs = key->tgsw_key->tlwe_key.key[0].coefs;
    for (int k = 0; k < n; ++k) {
        const uint32_t *a = (const uint32_t *)in + (size_t)k * 2 * kN, *b = a + kN;
        uint32_t *ph = (uint32_t *)phase + (size_t)k * kN;
        for (int j = 0; j < kN; ++j) ph[j] = b[j];
        for (int s = 0; s < kN; ++s) {
            if (!coefs[s]) continue;         // ph -= X^s * a (negacyclic)
            for (int i = 0; i < s; ++i) ph[i] += a[i - s + kN];
            for (int i = s; i < kN; ++i) ph[i] -= a[i - s];
        }
    }
    return TFHE_AMD_OK;
}

EXPORT TFheGateBootstrappingSecretKeySet *
new_random_gate_bootstrapping_secret_keyset(const TFheGateBootstrappingParameterSet *params) {
    const ParamsImpl *P = params_of(params);
    std::lock_guard<std::mutex> lk(g_rng_mu);
    LweKey *lwe_key = new_LweKey(params->in_out_params);
    lweKeyGen_nolock(lwe_key);                                              // :60
    TGswKeyImpl *gk = reinterpret_cast<TGswKeyImpl *>(new_tgsw_key(P));
    {   // tGswKeyGen -> tLweKeyGen (tlwe-functions.cu:15-23)
        std::uniform_int_distribution<int> distribution(0, 1);
        for (int j = 0; j < kN; ++j) gk->coefs[j] = distribution(generator);
    }
    // tfhe_createLweBootstrappingKey (lwe-bootstrapping-functions.cu:185-217)
    LweBootstrappingKey *bk = new_bk(P);
    create_ksk_nolock(bk->ks, gk->coefs.data(), lwe_key);   // extracted key = tlwe key coefs (k = 1)
    const double alpha = P->accum.alpha_min;
    for (int i = 0; i < kn; i++) {
        TGswSample *g = &bk->bk[i];
        for (int p = 0; p < kKpl; ++p) tlwe_encrypt_zero_nolock(&g->all_sample[p], alpha, gk->coefs.data());
        // tGswAddMuIntH (tgsw-functions.cu:114-124)
        for (int bloc = 0; bloc <= kK; ++bloc)
            for (int l = 0; l < kL; l++) {
                Torus32 *c0 = &g->bloc_sample[bloc][l].a[bloc].coefsT[0];
                *c0 = (Torus32)((uint32_t)*c0 + (uint32_t)lwe_key->key[i] * (uint32_t)P->h[l]);
            }
    }
    LweBootstrappingKeyFFT *bkfft = new_bkfft(bk);
    return new TFheGateBootstrappingSecretKeySet{params, lwe_key, &gk->pub,
                                                 TFheGateBootstrappingCloudKeySet{params, bk, bkfft}};
}

EXPORT void delete_gate_bootstrapping_secret_keyset(TFheGateBootstrappingSecretKeySet *keyset) {
    if (!keyset) return;
    delete_bkfft(const_cast<LweBootstrappingKeyFFT *>(keyset->cloud.bkFFT));
    delete_bk(const_cast<LweBootstrappingKey *>(keyset->cloud.bk));
    delete reinterpret_cast<TGswKeyImpl *>(const_cast<TGswKey *>(keyset->tgsw_key));
    delete_LweKey(const_cast<LweKey *>(keyset->lwe_key));
    delete keyset;
}

EXPORT void delete_gate_bootstrapping_cloud_keyset(TFheGateBootstrappingCloudKeySet *keyset) {
    if (!keyset) return;
    delete_bkfft(const_cast<LweBootstrappingKeyFFT *>(keyset->bkFFT));
    delete_bk(const_cast<LweBootstrappingKey *>(keyset->bk));
    delete keyset;
}

EXPORT void bootsSymEncrypt(LweSample *result, int message, const TFheGateBootstrappingSecretKeySet *key) {
    Torus32 _1s8 = modSwitchToTorus32(1, 8);
    Torus32 mu = message ? _1s8 : -_1s8;
    double alpha = key->params->in_out_params->alpha_min;
    lweSymEncrypt(result, mu, alpha, key->lwe_key);
}
EXPORT int bootsSymDecrypt(const LweSample *sample, const TFheGateBootstrappingSecretKeySet *key) {
    Torus32 mu = lwePhase(sample, key->lwe_key);
    return mu > 0 ? 1 : 0;
}

// ------------------------------------------------------------------ flat exports

EXPORT int tfhe_amd_export_bk(const TFheGateBootstrappingCloudKeySet *bk, int32_t *out) {
    if (!bk || !bk->bk || !out) return TFHE_AMD_E_ARG;
    bk_flatten(bk->bk, out);
    return TFHE_AMD_OK;
}
EXPORT int tfhe_amd_export_ksk(const TFheGateBootstrappingCloudKeySet *bk, int32_t *out) {
    if (!bk || !bk->bkFFT || !out) return TFHE_AMD_E_ARG;
    ksk_flatten(bk->bkFFT->ks, out);
    return TFHE_AMD_OK;
}
EXPORT int tfhe_amd_export_lwe_key(const TFheGateBootstrappingSecretKeySet *key, int32_t *out) {
    if (!key || !out) return TFHE_AMD_E_ARG;
    memcpy(out, key->lwe_key->key, sizeof(int32_t) * kn);
    return TFHE_AMD_OK;
}

EXPORT int tfhe_amd_export_tlwe_key(const TFheGateBootstrappingSecretKeySet *key, int32_t *out) {
    if (!key || !out) return TFHE_AMD_E_ARG;
    memcpy(out, key->tgsw_key->tlwe_key.key[0].coefs, sizeof(int32_t) * kN);
    return TFHE_AMD_OK;
}
int tfhe_amd_internal_bk_coef(const TFheGateBootstrappingCloudKeySet *bk, int32_t *out) {
    if (!bk || !bk->bkFFT || !out) return TFHE_AMD_E_ARG;
    memcpy(out, bk_coef_of(bk->bkFFT), sizeof(int32_t) * kn * kKpl * 2 * kN);
    return TFHE_AMD_OK;
}

// ------------------------------------------------------------------ L1 structs
// of the blind-rotation entry points (tier1.cpp)

struct TorusPolyImpl {
    TorusPolynomial pub;
    std::vector<Torus32> c;
};
struct TLweSampleImpl {
    TLweSample pub;
    std::vector<Torus32> coefs;
    std::vector<TorusPolynomial> polys;
};
// tlwe.h:222, polynomials.h:97 (allocation + construction; coefficients zero)
EXPORT TorusPolynomial *new_TorusPolynomial(const int N) {
    if (N <= 0) die_dramatically("new_TorusPolynomial: N must be positive");
    TorusPolyImpl *p = new TorusPolyImpl{TorusPolynomial{N, nullptr}, std::vector<Torus32>((size_t)N, 0)};
    p->pub.coefsT = p->c.data();
    return &p->pub;
}
EXPORT void delete_TorusPolynomial(TorusPolynomial *obj) { delete reinterpret_cast<TorusPolyImpl *>(obj); }
EXPORT TLweSample *new_TLweSample(const TLweParams *params) {
    const int k = params->k, N = params->N;
    TLweSampleImpl *t = new TLweSampleImpl{TLweSample{nullptr, nullptr, 0., k}, std::vector<Torus32>((size_t)(k + 1) * N, 0), {}};
    t->polys.reserve(k + 1);
    for (int i = 0; i <= k; ++i) t->polys.push_back(TorusPolynomial{N, t->coefs.data() + (size_t)i * N});
    t->pub.a = t->polys.data();
    t->pub.b = t->pub.a + k;
    return &t->pub;
}
EXPORT void delete_TLweSample(TLweSample *obj) { delete reinterpret_cast<TLweSampleImpl *>(obj); }
