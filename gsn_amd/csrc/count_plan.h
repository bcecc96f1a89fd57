// The counting launch as a plan: everything a counting entry point decides before it touches the device -- validation, routes, the LDS
// layout, staging, grid and kernel instantiation -- as one host function of the request, the host copy of the plan table and the
// environment switches.  Plain C++ (no HIP include): count_plan.cpp builds for the host alone, and tests/test_count_plan_cpu.py replays
// recorded launches through it without a GPU (tests/count_plan_harness.cpp, tests/golden/count_launch_plans.json).
#pragma once

#include "count_args.h"
#include "gsn_internal.h"

namespace gsn {

// What the counting entry points of the ABI ask for (include/gsn_abi.h: gsn_count_hip and its encode / pack16 / side / keys variants).
struct CountRequest {
    const uint32_t *plan_host = nullptr, *plan_dev = nullptr;
    int64_t plan_words = 0, n_graphs = 0;
    const int64_t *node_ptr = nullptr, *edge_ptr = nullptr, *edge_index = nullptr;
    int64_t edge_row_stride = 0;
    int ids_are_global = 0;
    const int32_t *graph_ids = nullptr;    // or null: every graph, n_items = n_graphs
    int64_t n_items = 0, max_nodes = 0, max_edges = 0;
    int64_t *out = nullptr;
    int32_t *status = nullptr;
    const int32_t *n_classes = nullptr;    // host, with enc_out
    int enc_clamp = 0;
    float *enc_out = nullptr;              // fp32 one-hot rows; with enc_no32 a placeholder that is never written
    uint16_t *enc16 = nullptr;             // fp16 row pack
    int64_t enc16_stride = 0, enc16_col0 = 0;
    int enc_no32 = 0;
    const gsn_count_side *side = nullptr;  // host
    const gsn_count_keys *keys = nullptr;  // host
};

// The environment switches of the counting launch (switches.h), with their defaults and clamps.
struct CountSwitches {
    int pull_batch = 8;             // GSN_PULL_BATCH, 1 .. 64
    bool pair = true;               // GSN_COUNT_PAIR
    int tail_loop = -1;             // GSN_COUNT_TAIL_LOOP: -1 by the capacities, 0 / 1 forced
    bool cycle = true;              // the cycle walk: GSN_COUNT_CYCLE and GSN_COUNT_MOL
    bool mol = true;                // the molecule instantiation: GSN_COUNT_MOL
    int64_t split_target = 2048;    // GSN_COUNT_SPLIT_TARGET
    bool enc_bytes = false;         // GSN_COUNT_ENC_BYTES
    static CountSwitches read();
};

enum CountKernel { GENERIC, GENERIC_TAIL, DIRECTED, DIRECTED_TAIL, MOL, CYCLE_ANY, CYCLE_KEYS };

struct CountLaunchPlan {
    CountArgs args;
    int W, T;               // count_kernel<W, T, ..>: 64-bit words per adjacency row, threads per workgroup
    CountKernel kernel;
    int grid;               // workgroups, side workgroups included; 0: nothing to launch
    int lds_bytes;
    bool memset_status;     // the status words are zeroed in front of the launch (else by their workgroups: args.zero_status)
};

// GSN_OK and *plan, or the refusal (set_error).  Reads host memory only: plan_host[0 .. plan_words), n_classes, *side, *keys; device
// pointers are tested for null and alignment and copied, never followed.
int count_plan(const CountRequest &rq, const CountSwitches &sw, CountLaunchPlan *plan);
// whether a launch meets the molecule instantiation's conditions (the cycle walk's are these and more); the launcher's trace line names it
bool count_molecule_route(const CountArgs &a, const CountSwitches &sw);

}  // namespace gsn
