// Every environment switch of libgsn_hip.so, stated once: its name, its lifetime and what it does.  Plain C++ (no HIP include), so
// the table and its readers build and test alone (tests/switches_harness.cpp).  getenv appears nowhere else in csrc/.
//
// Lifetime.  ONCE: the first read of the process is kept, later changes of the variable are not seen.  LIVE: read at every call
// (tests toggle these inside one process).  A row is LIVE when any site reads it live; the few sites that latch a LIVE switch in
// a function-local static of their own are named in the row.
//
// Readers.  The default belongs to the call site (one name may have two: GSN_SEG_PRIO), and so do clamps and other
// post-processing.  sw_int / sw_int64: unset -> default, else atoi / atoll.  sw_on: unset -> default, else atoi != 0.
// sw_present: set to anything, "0" and "" included.  sw_str: the raw text or nullptr (the sscanf lists, the one atof).
//
// Two rules differ from the code before this table, on purpose:
//   * GSN_CHAIN_TRACE is LIVE at every site (chain.hip used to latch atoi != 0 at its first launch while every other launcher tested
//     presence at each launch), and "present" is its one rule: tests set it to "1" and pop it again.
//   * GSN_EMBED_BWD_LDS and GSN_WGRAD_FP32 tested the first character for '1'; they are on/off switches like the rest (sw_on).
#pragma once

#include <cstdint>

namespace gsn {

enum SwitchLife { ONCE, LIVE };

// X(identifier, lifetime, description): the variable is GSN_<identifier>, the enumerator SW_<identifier>
#define GSN_SWITCH_TABLE(X)                                                                                                                \
    /* tracing */                                                                                                                          \
    X(CHAIN_TRACE, LIVE, "present: every launcher names the kernel it takes on stderr (gsn::trace)")                                       \
    /* chain kernels */                                                                                                                    \
    X(CHAIN_PERCU, LIVE, "int: workgroups per CU of mlp_chain_kernel (default 2 for small LDS footprints, else 1)")                        \
    X(CHAIN_DBG, LIVE, "int, default 0: ChainArgs::dbg ablation bits of mlp_chain_kernel")                                                 \
    X(CHAIN_PIPE, LIVE, "on/off, default on: 0 refuses the two-stage pipelined chain kernel")                                              \
    X(CHAIN_BF16X6, LIVE, "0 refuses the bf16x6 chain kernels; in chain_seg_bf16 the value is also the row tile (default 64)")             \
    X(CHAIN_SEGPIPE, LIVE, "int: row tile of the fp32 segment chain kernel, 0 refuses it")                                                 \
    X(PIPE_VEC4, LIVE, "on/off, default on: 16-byte staging loads of the bf16 pipe kernel")                                                \
    X(PIPE_PROF, LIVE, "on/off, default off: in-kernel phase clocks of the bf16 pipe kernel")                                              \
    X(SEG_PRIO, LIVE, "int: wave priority of the matrix phases; default 3 in chain_seg.hip, 0 in chain_seg_bf16.hip")                      \
    X(SEG_PROF, LIVE, "on/off, default off: in-kernel phase clocks of the segment chain kernels")                                          \
    X(SEG_VEC4, LIVE, "on/off, default on: 16-byte staging loads of the fp32 segment chain kernel")                                        \
    /* one-launch layer kernels */                                                                                                         \
    X(FUSED_GRID, LIVE, "int > 0: grid size of the layer kernels (fused, rr, rp, w, g) instead of their own choice")                       \
    X(FUSED_PRIO, ONCE, "int, default 1: wave priority of layer_fused_kernel's matrix phases")                                             \
    X(FUSED_ABLATE, LIVE, "int: ablation bits of layer_fused_kernel's profiling build (read with GSN_FUSED_PROF only)")                    \
    X(FUSED_GENERIC, LIVE, "present: layer_fused takes its generic instantiation")                                                         \
    X(FUSED_PROF, LIVE, "on/off, default off: in-kernel phase clocks; layer_rr / rp / w / g latch it at their first launch")               \
    X(FUSED_RR, ONCE, "int, default 1: 0 refuses layer_fused_kernel_rr")                                                                   \
    X(FUSED_W, ONCE, "int, default 1: 0 refuses layer_fused_kernel_w")                                                                     \
    X(FUSED_G, ONCE, "int, default 1: 0 refuses layer_fused_kernel_g")                                                                     \
    X(RP_OLD_SHARE, ONCE, "float, default 0.6: share of the grid that layer_fused_kernel_rp gives to its first range")                     \
    X(RP_TABLES, LIVE, "on/off, default on: 0 keeps layer_fused_kernel_rp on its KEYS arm where the step hands it x_i tables")             \
    /* linear layers */                                                                                                                    \
    X(LINEAR_SPLITK_RANGES, ONCE, "int, default -1 (automatic): forced split-k range count of the small bf16x6 linear, 0 = never")         \
    X(LINEAR_SMALL_MAX, ONCE, "int, default 96: most 128-row tiles that still take the 32-row-tile kernel, 0 = never")                     \
    X(LINEAR_BF16X6, ONCE, "on/off, default on: 0 selects the fp32-MFMA linear kernel")                                                    \
    X(LINEAR_VEC4, LIVE, "on/off, default on: float4 staging of A and W in the linear kernels")                                            \
    X(L16_SPLIT_WGS, ONCE, "int64, default 1024: workgroups of the fp16x3 row-split kernel, 0 = one tile per workgroup")                   \
    X(L16_WIDE, LIVE, "text, first character '1': 128 x 320 tiles in the fp16x3 linear where they fit (default off)")                      \
    X(L16_NOVEC, LIVE, "present: fp16x3 linear without 16-byte output stores")                                                             \
    X(L16_REGSTAGE, LIVE, "present: fp16x3 slices staged through registers; the planes launcher latches it at its first launch")           \
    X(L16_PROF, LIVE, "present: in-kernel phase clocks of the fp16x3 linear; the planes launcher latches it at its first launch")          \
    X(L16_DBG, LIVE, "int, default 0: ablation bits of the fp16x3 linear (1 no stores, 2 no products, 4 no loads)")                        \
    /* weight gradients and plane conversions */                                                                                           \
    X(BWD_PLANES_WGS, ONCE, "int64 > 0, default 2048: workgroups of the backward plane-split kernel")                                      \
    X(FWD_PLANES_WGS, ONCE, "int64 > 0, default 2048: workgroups of the forward plane-split kernel")                                       \
    X(WGRAD_WGS, ONCE, "int64 > 0, default 0 (automatic): workgroup target of a weight-gradient call's slabs")                             \
    X(WGRAD_FP32, ONCE, "on/off, default off: weight gradient by the fp32 kernel")                                                         \
    X(WGRAD_PIPE, ONCE, "int, default 6 (1 means 6): pipeline depth of the bf16 weight-gradient kernel, 0 = unpipelined")                  \
    X(WGRAD16_WGS, ONCE, "int64 > 0, default 0 (automatic): workgroup target of the fp16x3 weight gradient")                               \
    X(WGRAD16_VALU, ONCE, "int, default 3: VALU-side variant of the fp16x3 weight-gradient kernel")                                        \
    X(WGRAD16_DBG, LIVE, "int, default 0: ablation bits of the fp16x3 weight-gradient kernels")                                            \
    X(WGRAD16_DMA, LIVE, "text, first character '1': the LDS-DMA fp16x3 weight-gradient kernel (default off)")                             \
    /* counting */                                                                                                                         \
    X(COUNT_MOL, ONCE, "on/off, default on: molecule-sized instantiation of count_kernel")                                                 \
    X(COUNT_CYCLE, ONCE, "on/off, default on: cycle instantiation of count_kernel")                                                        \
    X(COUNT_PAIR, LIVE, "on/off, default on: two graphs per workgroup where the plan allows")                                              \
    X(COUNT_TAIL_LOOP, ONCE, "int, default -1 (by plan): forces the tail-loop instantiation on (1) or off (0)")                            \
    X(COUNT_SPLIT_TARGET, ONCE, "int64 > 0, default 2048: workgroup count below which large graphs are split")                             \
    X(COUNT_ENC_BYTES, ONCE, "present: keep the byte array beside staged counts")                                                          \
    X(PULL_BATCH, ONCE, "int, default 8, clamped to 1..64: cells a counting wave pulls at a time")                                         \
    /* encoders */                                                                                                                         \
    X(EMBED_NOVEC4, ONCE, "present: embedding kernels without 16-byte accesses")                                                           \
    X(EMBED_PIPE, ONCE, "on/off, default on: pipelined embedding sum kernel")                                                              \
    X(EMBED_LDS_MIN_ROWS, ONCE, "int64, default 8192: fewest rows that take the LDS embedding kernel")                                     \
    X(EMBED_BWD_LDS, ONCE, "on/off, default off: embedding backward by the LDS kernel only")                                               \
    /* propagation */                                                                                                                      \
    X(PROP_CP, LIVE, "list lpr,unr,blocks: forces one mapping of the pipelined propagate kernel, \"0\" the generic one")                   \
    X(PROP_RS, LIVE, "list lpr,unr,nt[,blocks]: forces one mapping of relu_sum3_kernel, \"0\" the generic kernel")                         \
    X(PROP_LPR, ONCE, "int, default 0 (by width): forced lanes per row of the propagate kernels")                                          \
    X(PROP_BWD_PIPE, ONCE, "on/off, default on: pipelined propagate backward kernels")                                                     \
    X(PROP_FOLD_SELF, ONCE, "on/off, default on: the self term folded into the propagate backward kernel")

enum Switch : int {
#define GSN_SWITCH_ENUM(id, life, what) SW_##id,
    GSN_SWITCH_TABLE(GSN_SWITCH_ENUM)
#undef GSN_SWITCH_ENUM
    SW_COUNT
};

struct SwitchRow {
    const char *name;
    SwitchLife life;
    const char *what;
};
const SwitchRow &switch_row(Switch s);

const char *sw_str(Switch s);                     // the text (a copy kept for the process if ONCE), nullptr when unset
int sw_int(Switch s, int dflt);
int64_t sw_int64(Switch s, int64_t dflt);
bool sw_on(Switch s, bool dflt);
bool sw_present(Switch s);

}  // namespace gsn
