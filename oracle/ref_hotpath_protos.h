// ref_hotpath_protos.h — TEST INFRASTRUCTURE ONLY (our own code, not reference code).
// What the reference's hot-path functions, cut out by oracle/extract_ref.py, and our driver need
// to see of each other.  The reference declares these in tfhe.h, tlwe_functions.h and
// tgsw_functions.h, which pull in cufftXt.h; every other header of the reference is included as
// it is.
#ifndef REF_HOTPATH_PROTOS_H
#define REF_HOTPATH_PROTOS_H
#include "tfhe_core.h"
#include "numeric_functions.h"
#include "polynomials.h"
#include "polynomials_arithmetic.h"
#include "lweparams.h"
#include "lwekey.h"
#include "lwesamples.h"
#include "lwe-functions.h"
#include "tlwe.h"
#include "tgsw.h"
#include "lwekeyswitch.h"
#include "lwebootstrappingkey.h"

// polynomials_arithmetic.h maps torusPolynomialAddMulR to this name; the driver defines it as the
// reference's exact Karatsuba product (the FFT file does not build here)
EXPORT void torusPolynomialAddMulRFFT(TorusPolynomial *result, const IntPolynomial *poly1, const TorusPolynomial *poly2);

EXPORT void tLweClear(TLweSample *result, const TLweParams *params);
EXPORT void tLweCopy(TLweSample *result, const TLweSample *sample, const TLweParams *params);
EXPORT void tLweNoiselessTrivial(TLweSample *result, const TorusPolynomial *mu, const TLweParams *params);
EXPORT void tLweAddTo(TLweSample *result, const TLweSample *sample, const TLweParams *params);
EXPORT void tLweAddMulRTo(TLweSample *result, const IntPolynomial *p, const TLweSample *sample, const TLweParams *params);
EXPORT void tLweMulByXaiMinusOne(TLweSample *result, int ai, const TLweSample *bk, const TLweParams *params);
EXPORT void tLweExtractLweSampleIndex(LweSample *result, const TLweSample *x, const int index, const LweParams *params,
                                      const TLweParams *rparams);
EXPORT void tLweExtractLweSample(LweSample *result, const TLweSample *x, const LweParams *params, const TLweParams *rparams);
EXPORT void tGswTorus32PolynomialDecompH(IntPolynomial *result, const TorusPolynomial *sample, const TGswParams *params);
EXPORT void tGswTLweDecompH(IntPolynomial *result, const TLweSample *sample, const TGswParams *params);
EXPORT void tGswExternMulToTLwe(TLweSample *accum, const TGswSample *sample, const TGswParams *params);
void tfhe_MuxRotate(TLweSample *result, const TLweSample *accum, const TGswSample *bki, const int barai,
                    const TGswParams *bk_params);
EXPORT void tfhe_blindRotate(TLweSample *accum, const TGswSample *bk, const int *bara, const int n, const TGswParams *bk_params);
EXPORT void tfhe_blindRotateAndExtract(LweSample *result, const TorusPolynomial *v, const TGswSample *bk, const int barb,
                                       const int *bara, const int n, const TGswParams *bk_params);
EXPORT void tfhe_bootstrap_woKS(LweSample *result, const LweBootstrappingKey *bk, Torus32 mu, const LweSample *x);
EXPORT void tfhe_bootstrap(LweSample *result, const LweBootstrappingKey *bk, Torus32 mu, const LweSample *x);
void lweKeySwitchTranslate_fromArray(LweSample *result, const LweSample ***ks, const LweParams *params, const Torus32 *ai,
                                     const int n, const int t, const int basebit);
#endif
