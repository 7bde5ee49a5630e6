// pack_key.h — the imported packing key, shared by pack.cpp (import, destroy, the
// pack calls) and acc.cpp (p-way selection, DESIGN.md §3.8, which packs into the key's own
// accumulator scratch).  Internal, not part of the C ABI.
#pragma once
#include <mutex>

#include "engine.h"

// The 3 000 key rows on `device` as 750 groups in the exact kernels' key layout (DeviceKey.bk_v2),
// 64 KB each, and the scratch of the calls on the key: the digit scratch of the pack calls, 2 MB per
// output of the largest batch so far, and the accumulator scratch of the selection calls, 8 KB per
// query of the largest batch so far.  Every call on the key shares them, so their reuse is ordered
// across streams like a set's tree scratch: grown under mu, fenced by `fence`.
struct TfheAmdPackKey {
    int device = -1;
    int cus = 0;   // compute units of the device: the split of the key rows is chosen from it
    uint32_t *v2 = nullptr;
    std::mutex mu;
    uint32_t *dig = nullptr;
    size_t dig_outputs = 0;
    int32_t *acc = nullptr;   // [acc_outputs][2][kN]
    size_t acc_outputs = 0;
    tfhe_amd::StreamFence fence;
};
