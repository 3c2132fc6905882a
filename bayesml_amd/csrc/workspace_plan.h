// The life cycle of a gmmvb_workspace as data: the switches it is created under, the shape derived from them, and ONE list
// of its device and pinned buffers that creation allocates from, gmmvb_workspace_bytes sums and destruction frees by.
//
// Plain C++: capi.hip fills KernelSizes from launch.h, binds the buffers to the workspace's fields (Slots) and
// runs allocate_all / free_all over an allocator that wraps hipMalloc and friends; tests/workspace_plan_cases.cpp runs the
// same code over malloc under ASan, failing every allocation in turn.  No HIP header here.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/gmmvb.h"

namespace gmmvb {

enum EstepVariant { kEstepLds = 0, kEstepDirect = 1, kEstepLds8 = 2, kEstepI8 = 3, kEstepValu16 = 4 };
inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// ---- switches ------------------------------------------------------------------------------------------------------------
// Two are part of the interface: GMMVB_ESTEP_PRUNE and GMMVB_MSTEP_SPARSE.  Every other GMMVB_* switch is a
// test / developer seam - it selects between kernels whose results agree, so that a parity test can run each of them - and
// is only looked at when GMMVB_DEBUG is set ("1"; "2" also prints one line per E-step on stderr).  All of them are read once,
// when a workspace / HMM state is created (no getenv on the per-iteration path).
inline bool not_zero(const char* v) { return !(v && std::strcmp(v, "0") == 0); }
inline bool is(const char* v, const char* word) { return v && std::strcmp(v, word) == 0; }
template <typename Lookup>
inline const char* dev_switch(Lookup&& lookup, const char* name) {
    const char* on = lookup("GMMVB_DEBUG");
    return (on && on[0] != '\0' && on[0] != '0') ? lookup(name) : nullptr;
}

struct WorkspaceOptions {
    bool sparse = true;                // GMMVB_MSTEP_SPARSE=0: always the dense M-step
    int prune = 1;                     // GMMVB_ESTEP_PRUNE: "0" never (0), "force" always (2), else by the policy (1)
    int variant_asked = -1;            // GMMVB_ESTEP_VARIANT=lds8|direct|lds4|i8 (-1: the shape's default)
    bool sort_rows = true;             // GMMVB_SORT_ROWS=0: never regroup
    double settle_margin = 1e300;      // GMMVB_SETTLE_MARGIN: nats; negative = never settle rows
    bool opt_proof = true;             // GMMVB_PROOF=0: no int8 proof round (rows then never settle)
    bool opt_proof_all = true;         // GMMVB_PROOF=settled: only the settled rows' pairs go through it
    bool opt_proof_blocked = true;     // GMMVB_PROOF_BLOCKED=0: estep_i8_proof, component after component, not the row superblocks
    bool opt_lazy = true;              // GMMVB_SWEEP_LAZY=0: every sweep reads all K bounds of every row
    // the stateless table of project.h - off by default (measured, profiles/r6_experiments.md: on the benchmark's fits it
    // costs more than the proof pairs it saves): "filter" (1) = it takes pairs off the carried sweep's proof lists, "only"
    // (2) = it replaces the carried per-pair bounds
    int opt_project = 0;
    bool opt_regroup_margin = true;    // GMMVB_REGROUP_MARGIN=0: the rows are regrouped by best component only
    bool gather_exit = true;           // GMMVB_GATHER_EXIT=0: candidates are always evaluated in full
    bool cache_on = true;              // GMMVB_MSTEP_CACHE=0: no cache of single-component rows
    bool opt_carry_off = false;        // GMMVB_ESTEP_CARRY_OFF (set at all): ignore gmmvb_set_drift
    bool opt_hmm_mstep_dense = false;  // GMMVB_HMM_MSTEP_DENSE (set at all): the HMM's small M-step walks every (step, state)
    bool opt_calibrate = true;         // GMMVB_POLICY_CALIBRATE=0: the scaled literals only
    bool opt_quiet_tiles = true;       // GMMVB_QUIET_TILES=0: no tile-level shortcuts for tiles of settled rows (workspace.h)
    bool opt_mlist_xc = false;         // GMMVB_MLIST_XC=1: the list M-step reads the centred f64 copy, never f32 rows (mstep_plan.h)
    int opt_mlist_runs = 0;            // GMMVB_MLIST_RUNS=<n>: at most n runs in the list M-step (mstep.h); 0: what the device holds
    int opt_sweep_run = 0;             // GMMVB_SWEEP_RUN=<n>: the carried sweep's workgroups take runs of n tiles (records.h; the
                                       // compiled length nearest below n, 1 = a tile per workgroup); 0: what the shape's default is
    bool opt_debug = false;            // GMMVB_DEBUG=2

    // lookup: const char* (const char* name), null for an unset name - std::getenv in the library
    template <typename Lookup>
    static WorkspaceOptions read(Lookup&& lookup) {
        auto dev = [&lookup](const char* name) { return dev_switch(lookup, name); };
        WorkspaceOptions o;
        o.sparse = not_zero(lookup("GMMVB_MSTEP_SPARSE"));
        o.prune = is(lookup("GMMVB_ESTEP_PRUNE"), "0") ? 0 : (is(lookup("GMMVB_ESTEP_PRUNE"), "force") ? 2 : 1);
        const char* variant = dev("GMMVB_ESTEP_VARIANT");
        o.variant_asked = is(variant, "lds8") ? kEstepLds8 : is(variant, "direct") ? kEstepDirect : is(variant, "lds4") ? kEstepLds
                          : is(variant, "i8") ? kEstepI8 : -1;
        o.sort_rows = not_zero(dev("GMMVB_SORT_ROWS"));
        if (const char* v = dev("GMMVB_SETTLE_MARGIN")) o.settle_margin = std::atof(v);
        o.opt_proof = not_zero(dev("GMMVB_PROOF"));
        o.opt_proof_all = !is(dev("GMMVB_PROOF"), "settled");
        o.opt_proof_blocked = not_zero(dev("GMMVB_PROOF_BLOCKED"));
        o.opt_lazy = not_zero(dev("GMMVB_SWEEP_LAZY"));
        o.opt_project = is(dev("GMMVB_PROJECT"), "filter") ? 1 : (is(dev("GMMVB_PROJECT"), "only") ? 2 : 0);
        o.opt_regroup_margin = not_zero(dev("GMMVB_REGROUP_MARGIN"));
        o.gather_exit = not_zero(dev("GMMVB_GATHER_EXIT"));
        o.cache_on = not_zero(dev("GMMVB_MSTEP_CACHE"));
        o.opt_carry_off = dev("GMMVB_ESTEP_CARRY_OFF") != nullptr;
        o.opt_hmm_mstep_dense = dev("GMMVB_HMM_MSTEP_DENSE") != nullptr;
        o.opt_calibrate = not_zero(dev("GMMVB_POLICY_CALIBRATE"));
        o.opt_quiet_tiles = not_zero(dev("GMMVB_QUIET_TILES"));
        if (const char* v = dev("GMMVB_MLIST_XC")) o.opt_mlist_xc = v[0] == '1';
        if (const char* v = dev("GMMVB_MLIST_RUNS")) o.opt_mlist_runs = std::max(0, std::atoi(v));
        if (const char* v = dev("GMMVB_SWEEP_RUN")) o.opt_sweep_run = std::max(0, std::atoi(v));
        o.opt_debug = lookup("GMMVB_DEBUG") && lookup("GMMVB_DEBUG")[0] == '2';
        return o;
    }
};

// The carried sweep's run length (records.h: tiles per workgroup, and per addition to the opened-columns counter) as a
// compile-time constant: 1, 2 or 4, at one and two mask words.  At three and four (K > 128) the one-tile form already
// holds 96 registers and the written-out run goes to scratch: a tile per workgroup there, always.  GMMVB_SWEEP_RUN=n
// (developer switch) picks the compiled length nearest below n.
constexpr int kSweepRunDefault = 2;      // (measured, profiles/sweep_chain.md: 4 costs a resident workgroup and gains nothing more)
inline int sweep_run_length(int K, int asked) {
    if (K > 128) return 1;
    const int want = asked > 0 ? asked : kSweepRunDefault;
    return want >= 4 ? 4 : (want >= 2 ? 2 : 1);
}
template <typename F>
inline void dispatch_sweep_run(int run, F&& f) {
    if (run == 4) return f(std::integral_constant<int, 4>{});
    if (run == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 1>{});
}

// ---- shape ---------------------------------------------------------------------------------------------------------------
// Sizes that live in the kernels' translation units, as numbers: the constants, then the values at this (K, D) and its tile
// count (capi.hip: kernel_sizes; a generic shape, D > 32 max_tiles, only has the constants and generic_rows).
struct KernelSizes {
    int max_tiles = 0, t1_splits = 0, sel_rows = 0, lse_rows = 0, scan_parts = 0, rec_slots = 0;
    int mstep_components_per_wg = 0;       // the smaller of the two forms: sizes the slabs
    int slab_len = 0, estep_image_doubles = 0, estep_tri_image_doubles = 0, estep_bound_blocks = 0;
    int estep_i8_image_bytes = 0, estep_i8_bound_image_bytes = 0;
    int64_t estep_i8_digit_row_bytes = 0, proj_image_len = 0, proj_const_len = 0;
    int generic_rows = 0;
};

// 16 features per tile.  max_tiles < T <= 2 max_tiles (128 < D <= 256, round 4): dense MFMA kernels of their own - the
// E-step streams U's block rows through LDS (estep_rows.h), the M-step spreads a component's tile pairs over T / 2 waves
// (mstep.h) - instantiated for even tile counts: an odd one is rounded up (zero padded images and centred rows).
inline bool wide_features(int D, int max_tiles) { return D > 16 * max_tiles && D <= 32 * max_tiles; }
inline int feature_tiles(int D, int max_tiles) {
    const int T = (D + 15) / 16;
    return wide_features(D, max_tiles) ? 2 * ((T + 1) / 2) : T;
}

// What a workspace is created as (gmmvb_workspace derives from it): the switches in force - sparse, prune, sort_rows and
// cache_on after the vetoes of make_shape - and everything derived from them and the arguments before anything is allocated.
struct WorkspaceShape : WorkspaceOptions {
    int K = 0, D = 0, x_dtype = 0, num_cu = 0, T = 0;
    int64_t max_rows = 0, npad = 0;
    bool wide = false;                 // no pruning, no lists, K-side through torch
    bool generic = false;              // more than 2 max_tiles feature tiles: the plain f64 kernels of generic.h
    int KG = 0, S_cap = 0, img_len = 0, estep_variant = 0, gen_S = 1, img_i8_len = 0, img_i8b_len = 0;
    int64_t split_rows = 0, xc_len = 0;
    bool has_lists = false;            // sample lists, records, masks and the rest of the pruned / sparse machinery
};

inline WorkspaceShape make_shape(int K, int D, int x_dtype, int64_t max_rows, int num_cu, const WorkspaceOptions& opt,
                                 const KernelSizes& ks) {
    WorkspaceShape s;
    s.K = K;
    s.D = D;
    s.x_dtype = x_dtype;
    s.max_rows = max_rows;
    s.num_cu = num_cu;
    s.T = feature_tiles(D, ks.max_tiles);
    s.wide = wide_features(D, ks.max_tiles);
    s.generic = D > 32 * ks.max_tiles;
    s.npad = round_up(max_rows, 64);
    if (s.generic) {                   // no parameter images, no pruning, no lists, and no switch is looked at
        s.sparse = s.sort_rows = s.cache_on = false;
        s.prune = 0;
        s.gen_S = (int)std::min<int64_t>(64, std::max<int64_t>(1, max_rows / 16384));
        return s;
    }
    static_cast<WorkspaceOptions&>(s) = opt;
    s.KG = (K + ks.mstep_components_per_wg - 1) / ks.mstep_components_per_wg;
    // row splits of the dense M-step: ~4 workgroups per CU; with a single feature tile a step is a row load and one
    // MFMA - latency, not arithmetic - so many more, shorter, splits (HMM config 5; 24: three of the HMM
    // M-step's 50-KB workgroups per CU)
    s.S_cap = std::max(8, (int)round_up(((int64_t)(s.T == 1 ? ks.t1_splits : 4) * num_cu + s.KG - 1) / s.KG, 8));
    // Cap on the rows of one M-step split: 16 MB of centred rows (16384 rows at D = 128).  All component groups
    // of a split stream the same rows; short splits keep those workgroups within an L2's reach of each other
    // (measured at C3: fetch 96 GB -> 16-21 GB ~ the algorithmic 15.4 GB, kernel 175.6 -> 171.5 ms) at the
    // price of more slabs (+0.7 ms reduce).
    s.split_rows = round_up(std::max<int64_t>(64, (16 << 20) / (16 * s.T * 8)), 64);
    s.S_cap = (int)std::max<int64_t>(s.S_cap, round_up((max_rows + s.split_rows - 1) / s.split_rows, 8));
    s.img_len = ks.estep_image_doubles;
    // kEstepLds8 is measured fastest (two waves per SIMD share one LDS image) ... except with a single feature tile
    // (D <= 16): the 2.5-KB images stay in L1, staging them through LDS with a barrier per group of components only costs
    // (HMM config 5: emission 4.4 -> 3.1 ms), and the vector ALU, which can skip U's upper triangle, beats the matrix pipe
    // (estep.h, estep_rows16_f64: HMM emission 3.1 -> 2.7 ms); GMMVB_ESTEP_VARIANT=direct keeps the MFMA kernel.  One
    // E-step kernel past max_tiles feature tiles.
    s.estep_variant = s.T == 1 ? kEstepValu16 : kEstepLds8;
    if (!s.wide && opt.variant_asked >= 0) s.estep_variant = opt.variant_asked;
    // the sample lists hold 32-bit row numbers; dense kernels only when wide; one component: r = 1 for every row, nothing to
    // prune, list or cache
    if (max_rows > 2000000000 || s.wide || K == 1) s.sparse = false;
    if (max_rows > 2000000000) s.sort_rows = false;
    if (!s.sparse || ks.estep_bound_blocks == 0 || K > 256) s.prune = 0;
    // ... and the one-pass moment computation of multivariate_normal.LearnModel (K = 1, unit responsibilities) should not
    // pay for a centred copy it never builds: the M-step reads x directly (wide: it only exists over the centred copy)
    s.xc_len = (K == 1 && !s.wide) ? 0 : (s.npad + 64) * 16 * (int64_t)s.T;
    s.has_lists = s.sparse && K <= 256;
    if (s.estep_variant == kEstepI8) s.img_i8_len = ks.estep_i8_image_bytes;
    if (s.prune != 0) s.img_i8b_len = ks.estep_i8_bound_image_bytes;
    return s;
}

// ---- the buffers ---------------------------------------------------------------------------------------------------------
// Every device and pinned buffer a workspace is created with, by the name of its field in gmmvb_workspace.
#define GMMVB_WORKSPACE_BUFFERS(X)                                                                                             \
    X(tri) X(img_i8) X(img_i8b) X(pivot_i8) X(lnrho) X(lse) X(img) X(cvec) X(pivot) X(slabs) X(xc) X(dpart) X(thr) X(apart)     \
    X(ctr) X(drift) X(lists) X(khat) X(counts) X(plan) X(plan_m) X(blk) X(scan_parts) X(masks) X(lock) X(lcomp) X(dlock)       \
    X(rthr) X(exit_ctr) X(exit_host) X(dmask) X(dblk) X(mmask) X(rmask) X(rblk) X(mblk) X(cache) X(spart) X(gpart) X(qpart)    \
    X(epart) X(opart) X(mpart) X(ppart) X(xq) X(xqe) X(gimg) X(gconst) X(tile_ref) X(rec_k) X(rec_d) X(rec_B) X(rec_exact)    \
    X(rec_sel) X(rec_flags) X(ub32) X(tmeta) X(xp) X(perm) X(iperm) X(perm_tmp) X(gen_u) X(gen_m) X(gen_first) X(gen_second)  \
    X(ctr_host)
#define GMMVB_X(name) kBuf_##name,
enum BufferId { GMMVB_WORKSPACE_BUFFERS(GMMVB_X) kBufCount };
#undef GMMVB_X
#define GMMVB_X(name) #name,
inline const char* buffer_name(int id) {
    static const char* const names[kBufCount] = {GMMVB_WORKSPACE_BUFFERS(GMMVB_X)};
    return names[id];
}
#undef GMMVB_X

enum : unsigned {
    kZeroed = 1,       // zeroed at creation, right behind its allocation ...
    kZeroedLast = 8,   // ... or once everything is allocated (the order in which creation has always issued its fills)
    kPinned = 2,       // pinned host memory (not counted in gmmvb_workspace_bytes)
    kScratch = 4,      // belongs to the tile group (Scratch), not to the workspace
};
struct BufferSpec {
    int id;
    int64_t bytes;
    unsigned flags;
    int code;                  // what gmmvb_workspace_create answers when this allocation fails
    const char* what;
    bool counted() const { return (flags & kPinned) == 0; }
};

// In the order in which they are allocated (a workspace's device layout follows from it).  A buffer of no bytes is left out.
struct BufferPlan : std::vector<BufferSpec> {
    int code = GMMVB_ENOMEM;
    const char* what = "";
    void group(int c, const char* w) { code = c, what = w; }
    void add(int id, int64_t bytes, unsigned flags = 0) {
        if (bytes > 0) push_back(BufferSpec{id, bytes, flags, code, what});
    }
    int64_t counted_bytes() const {
        int64_t sum = 0;
        for (const BufferSpec& b : *this) sum += b.counted() ? b.bytes : 0;
        return sum;
    }
};

// group_npad: the padded rows of the tile group's first workspace, which sizes the group's sample lists (0: this is it)
inline BufferPlan buffer_plan(const WorkspaceShape& s, const KernelSizes& ks, int64_t group_npad = 0) {
    const int64_t K = s.K, D = s.D, np = s.npad, f64 = 8, i32 = 4;
    BufferPlan p;
    if (s.generic) {
        p.group(GMMVB_ENOMEM, "hipMalloc (workspace)");
        p.add(kBuf_lnrho, K * np * f64, kScratch);
        p.add(kBuf_lse, np * f64);
        p.add(kBuf_cvec, K * f64);
        p.add(kBuf_pivot, D * f64, kZeroedLast);
        p.add(kBuf_gen_u, K * D * D * f64);
        p.add(kBuf_gen_m, K * D * f64);
        p.add(kBuf_gen_first, s.gen_S * K * (D + 2) * f64);
        p.add(kBuf_gen_second, s.gen_S * K * (s.T * (s.T + 1) / 2) * 256 * f64);
        p.add(kBuf_ctr, 8 * f64, kZeroedLast);
        p.group(GMMVB_EHIP, "workspace initialisation");
        p.add(kBuf_ctr_host, 8 * f64, kPinned);
        return p;
    }
    const int64_t blocks = (np + ks.sel_rows - 1) / ks.sel_rows, words = (K + 63) / 64;
    p.group(GMMVB_ENOMEM, "hipMalloc (packed triangular images)");
    if (s.estep_variant == kEstepValu16) p.add(kBuf_tri, K * ks.estep_tri_image_doubles * f64);
    p.group(GMMVB_ENOMEM, "hipMalloc (int8 images)");
    p.add(kBuf_img_i8, K * s.img_i8_len);
    p.add(kBuf_img_i8b, K * s.img_i8b_len);
    if (s.img_i8_len || s.img_i8b_len) p.add(kBuf_pivot_i8, D * f64);
    p.group(GMMVB_ENOMEM, "hipMalloc (workspace)");
    p.add(kBuf_lnrho, K * np * f64, kScratch);
    p.add(kBuf_lse, np * f64);
    p.add(kBuf_img, K * s.img_len * f64);
    p.add(kBuf_cvec, K * f64);
    p.add(kBuf_pivot, D * f64, kZeroedLast);
    p.add(kBuf_slabs, s.S_cap * K * ks.slab_len * f64, kScratch);
    p.add(kBuf_xc, s.xc_len * f64, kScratch);
    p.add(kBuf_dpart, (np + ks.lse_rows - 1) / ks.lse_rows * K * f64);
    p.add(kBuf_thr, K * f64);
    p.add(kBuf_apart, blocks * f64);
    p.add(kBuf_ctr, 8 * f64, kZeroedLast);
    p.add(kBuf_drift, 4 * K * f64);
    if (s.has_lists) {
        // sample lists of the pruned E-step and the sparse M-step (one set for the tile group), gather plans, block counts
        // and their scan parts, four sets of masks, the settled rows and their cache, per-block counters, the records
        p.group(GMMVB_ENOMEM, "hipMalloc (sample lists / records)");
        p.add(kBuf_lists, K * (group_npad ? group_npad : np) * i32, kScratch);
        p.add(kBuf_khat, np * i32);
        p.add(kBuf_counts, K * i32);
        p.add(kBuf_plan, (K + 1) * i32);
        p.add(kBuf_plan_m, (K + 2) * i32);
        p.add(kBuf_blk, blocks * K * i32);
        p.add(kBuf_scan_parts, K * ks.scan_parts * i32);
        p.add(kBuf_masks, words * np * 8);
        p.add(kBuf_lock, np, kZeroed);
        p.add(kBuf_lcomp, np);
        p.add(kBuf_dlock, np * 4);
        p.add(kBuf_rthr, np * 4);
        p.add(kBuf_exit_ctr, 4 * 8, kZeroed);
        p.add(kBuf_exit_host, 4 * 8, kPinned | kZeroed);
        p.add(kBuf_dmask, words * np * 8);
        p.add(kBuf_dblk, blocks * K * i32);
        p.add(kBuf_mmask, words * np * 8);
        p.add(kBuf_rmask, words * np * 8);
        p.add(kBuf_rblk, blocks * K * i32);
        p.add(kBuf_mblk, blocks * K * i32);
        p.add(kBuf_cache, K * (2 + D + D * D) * f64, kZeroed);
        for (int id : {kBuf_spart, kBuf_gpart, kBuf_qpart, kBuf_epart, kBuf_opart, kBuf_mpart}) p.add(id, blocks * f64);
        p.add(kBuf_ppart, blocks * f64, kZeroed);
        if (s.prune != 0 && s.opt_proof && s.cache_on) {      // the proof round's digit planes
            p.add(kBuf_xq, np * ks.estep_i8_digit_row_bytes);
            p.add(kBuf_xqe, np);
            // the stateless sweep's table (project.h): needs the digit planes, regrouped rows and at least two feature blocks
            if (s.opt_project != 0 && s.sort_rows && K <= ks.sel_rows && D > 32 && D <= 128) {
                p.add(kBuf_gimg, ks.proj_image_len, kZeroed);
                p.add(kBuf_gconst, ks.proj_const_len * 16);
                p.add(kBuf_tile_ref, blocks * i32);
            }
        }
        p.add(kBuf_rec_k, ks.rec_slots * np * 2);
        p.add(kBuf_rec_d, ks.rec_slots * np * 4);
        p.add(kBuf_rec_B, np * 4);
        for (int id : {kBuf_rec_exact, kBuf_rec_sel, kBuf_rec_flags}) p.add(id, np);
        p.add(kBuf_ub32, K * np * 4);
        if (s.opt_lazy && K <= ks.sel_rows) p.add(kBuf_tmeta, blocks * K * 16);      // the lazy sweep's state per tile and component
        if (s.sort_rows) {
            p.add(kBuf_xp, s.max_rows * D * (s.x_dtype == GMMVB_F64 ? 8 : 4));
            for (int id : {kBuf_perm, kBuf_iperm, kBuf_perm_tmp}) p.add(id, np * i32);
        }
    }
    p.group(GMMVB_EHIP, "workspace initialisation");
    p.add(kBuf_ctr_host, 8 * f64, kPinned);
    return p;
}

// ---- allocation ----------------------------------------------------------------------------------------------------------
// The kScratch buffers of a tile group (workspace.h: gmmvb_scratch).  The first workspace that needs one allocates it for
// the group; a further tile borrows it and must not need more; the last reference frees them.
struct Scratch {
    void* buf[kBufCount] = {};
    int64_t bytes[kBufCount] = {};
    int64_t npad = 0;                  // padded rows of the group's first workspace
    int refs = 0;
};
using BufferSlots = void** const*;     // [kBufCount]: where the workspace keeps each buffer's pointer

// Allocator: void* get(bytes, pinned) (null: failed), bool zero(p, bytes, pinned), void release(p, pinned).
// Returns the entry that could not be had, or null.  What the call did get stays in the slots and in the group: free_all
// releases it (a further tile was refused before anything was allocated for it).
template <typename Allocator>
const BufferSpec* allocate_all(const BufferPlan& plan, BufferSlots slots, Scratch* group, Allocator& a, int64_t* counted) {
    static const BufferSpec too_large{-1, 0, 0, GMMVB_EINVAL, "a further tile must not be larger than the group's first workspace"};
    for (const BufferSpec& b : plan)
        if ((b.flags & kScratch) && group->buf[b.id] && b.bytes > group->bytes[b.id]) return &too_large;
    for (const BufferSpec& b : plan) {
        void*& p = *slots[b.id];
        if ((b.flags & kScratch) && group->buf[b.id]) {
            p = group->buf[b.id];
            continue;
        }
        p = a.get(b.bytes, (b.flags & kPinned) != 0);
        if (!p) return &b;
        if (b.flags & kScratch) {
            group->buf[b.id] = p;
            group->bytes[b.id] = b.bytes;
        }
        if (b.counted()) *counted += b.bytes;
        if ((b.flags & kZeroed) && !a.zero(p, b.bytes, (b.flags & kPinned) != 0)) return &b;
    }
    static const BufferSpec initialisation{-1, 0, 0, GMMVB_EHIP, "workspace initialisation"};
    for (const BufferSpec& b : plan)
        if ((b.flags & kZeroedLast) && !a.zero(*slots[b.id], b.bytes, false)) return &initialisation;
    return nullptr;
}

// Releases what the workspace owns and its reference to the group.  True: that was the last one, the group's buffers are
// freed and the caller disposes of the group object.
template <typename Allocator>
bool free_all(const BufferPlan& plan, BufferSlots slots, Scratch* group, Allocator& a) {
    for (const BufferSpec& b : plan) {
        void*& p = *slots[b.id];
        if (p && !(b.flags & kScratch)) a.release(p, (b.flags & kPinned) != 0);
        p = nullptr;
    }
    if (!group || --group->refs > 0) return false;
    for (void*& p : group->buf) {
        if (p) a.release(p, false);
        p = nullptr;
    }
    return true;
}

}  // namespace gmmvb
