// tgsw_internal.h — what the leveled mode's host modules share (tgsw.cpp, tgsw_dfa.cpp): the imported
// set and the staging buffers of the host forms.  Not installed.
#pragma once
#include <mutex>
#include <vector>

#include "engine.h"

// `count` samples on `device` in the exact kernels' key layout (DeviceKey.bk_v2), 64 KB each, and
// the CMux tree's scratch: two buffers the levels alternate between, shared by every lookup on
// the set, so their reuse is ordered across streams like a context's extracted samples.
struct TfheAmdTgsw {
    int device = -1;
    int count = 0;
    uint32_t *v2 = nullptr;
    std::mutex mu;
    int32_t *tree = nullptr;
    size_t tree_words = 0;
    tfhe_amd::StreamFence fence;
};

namespace tfhe_amd {

// temporary device buffers of the host forms, freed on every path
struct DevBufs {
    std::vector<void *> p;
    ~DevBufs() {
        for (void *q : p) (void)hipFree(q);
    }
    template <class T>
    hipError_t get(T **out, size_t words) {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, sizeof(T) * (words ? words : 1));
        if (e == hipSuccess) p.push_back(q);
        *out = static_cast<T *>(q);
        return e;
    }
};

}  // namespace tfhe_amd
