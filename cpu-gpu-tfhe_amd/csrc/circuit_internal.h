// circuit_internal.h — what circuit.cpp (compiler and runner) and circuit_select.cpp (the select part
// of a run) share.  Internal, not part of the C ABI.
//
// circuit.cpp names no launcher of the pack, the box fill or the tlwe rows rotation: the
// ThreadSanitizer build links it against stand-in kernels that end at the launchers the circuit engine
// had before select nodes.  The runner reaches the select part of a level through the hook below, which
// is null on every path but tfhe_amd_circuit_run_pk_dev (circuit_select.cpp).  In the same way it
// names none of the mixed-key launchers: a key ring's run (keyring_circuit.cpp) takes
// each level's rotation and key switch through the level hook, null on every other path.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "engine.h"

struct TfheAmdCircuit;

namespace tfhe_amd {

// The select rows of one level as the runner hands them to the hook.  The rows are grouped by p (rows
// of one p are consecutive), in the order of h_sel / d_sel / d_rows; select row r at instance k has u
// slot and guard flags r B + k of the arrays given here, which are the level's own behind its other
// u rows.
struct CircSelLevel {
    int B, nsel, n_wires;
    const CircSel *h_sel;    // host copy of the records (the hook reads each row's p)
    const CircSel *d_sel;    // the records on the device
    const CircRow *d_rows;   // the rows' selectors on the device
    const int32_t *wa, *wb;  // the wire table
    int32_t *u_a, *u_b;
    Guard guard;             // flags null: unguarded
};
// Enqueues pack, box fill and rotation of the level's select rows on s; a TFHE_AMD_* code.
struct CircSelectHook {
    int (*fn)(void *arg, const DeviceKey &key, const CircSelLevel &lv, hipStream_t s);
    void *arg;
};

// One bootstrapped level as the runner hands it to the level hook (mixed-key runs, DESIGN.md §3.13,
// keyring_circuit.cpp): the hook enqueues the level's rotation (u slot and guard flags r B + k) and its
// key switch in place of the runner's own two launches; the runner keeps the linear launch.
struct CircLevelJob {
    int level;               // index into the circuit's levels (tfhe_amd_internal_circuit_levels)
    int B, nrows, nks;
    BrMode mode;
    const CircRow *d_rows;   // the level's rows and key-switch records on the device
    const CircKs *d_ks;
    int32_t *wa, *wb;        // the wire table
    int32_t *u_a, *u_b;
    Guard guard;             // flags null: unguarded
};
struct CircLevelHook {
    int (*fn)(void *arg, const CircLevelJob &lv, hipStream_t s);
    void *arg;
    uint64_t schedule;   // the schedule the hook's caller planned against (tfhe_amd_internal_circuit_levels)
};

}  // namespace tfhe_amd

// tfhe_amd_circuit_run_dev_impl with the hook; hook = null refuses a circuit that holds a select node
// (TFHE_AMD_E_ARG, before anything is launched)
int tfhe_amd_circuit_run_dev_hook(uint64_t ctx_uid, const tfhe_amd::DeviceKey &key, int device, hipStream_t s,
                                  TfheAmdCircuit *c, int B, int32_t *wa, int32_t *wb, uint32_t *guard_stats,
                                  const tfhe_amd::CircSelectHook *hook);
// the same with the level hook, which is null on every path but the key ring's: ctx_uid is then the
// ring's own id, under which the level tables and the u scratch are kept
int tfhe_amd_circuit_run_dev_hooks(uint64_t ctx_uid, const tfhe_amd::DeviceKey &key, int device, hipStream_t s,
                                   TfheAmdCircuit *c, int B, int32_t *wa, int32_t *wb, uint32_t *guard_stats,
                                   const tfhe_amd::CircSelectHook *hook, const tfhe_amd::CircLevelHook *level_hook);
// What a level hook's caller plans against, in one locked query: compiles the circuit if need be and
// gives the key-switched outputs of each level, whether a select node is held, and the schedule's
// number.  A run whose hook names another number (the circuit was recompiled in between) is refused by
// the runner with TFHE_AMD_E_ARG before anything is launched.  Returns a TFHE_AMD_* code.
int tfhe_amd_internal_circuit_levels(TfheAmdCircuit *c, std::vector<int> *nks, int *has_select, uint64_t *schedule);
