// Workspace object and error helper shared by the C-ABI translation units.
#pragma once
#include "../../include/gmmvb.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "pass_plan.h"
#include "workspace_plan.h"

struct gmmvb_hmm_state;      // HMM forward-backward buffers (hmm_capi.hip), allocated by hmmvb_enable
struct gmmvb_workspace;

// Buffers that only live from an E-step to the M-step (or read-out) behind it: ln rho [K][npad] f64, the sample lists
// [K][npad] i32, the centred f64 copy of the rows and the M-step's slabs - 3.5 KB per row at K = 256, D = 64, two thirds of
// the workspace.  The workspaces of ONE row-tiled job (gmmvb_workspace_create_tile) share one set, sized for the largest
// tile: what a tile carries from iteration to iteration (f32 bounds, records, digit planes, settled rows, row order) stays
// its own.  `owner` is the workspace whose E-step output the buffers hold; another workspace that needs them takes them
// over (capi.hip: claim_scratch) and the previous owner is back to "no E-step output".  All on one stream.
struct gmmvb_scratch : gmmvb::Scratch {   // buf[kBuf_lnrho], [kBuf_xc], [kBuf_slabs], [kBuf_lists], their bytes, npad, refs
    gmmvb_workspace* owner = nullptr;
};

// K, D, T, the sizes derived from them and every switch are the shape the workspace was created as (workspace_plan.h)
struct gmmvb_workspace : gmmvb::WorkspaceShape {
    gmmvb_scratch* scratch = nullptr;  // lnrho / xc / slabs / lists below point into it
    bool lost_estep = false;           // the last E-step's output went to another tile of the group (e_state 0); its counters,
                                       // masks and block counts are still that pass's
    double* lnrho = nullptr;   // [K][npad]
    double* lse = nullptr;     // [npad]
    double* img = nullptr;     // [K][img_len] parameter images (layout: estep.h)
    double* tri = nullptr;             // [K][estep_tri_image_doubles()] packed lower-triangular images (D <= 16: estep_rows16_f64)
    unsigned char* img_i8 = nullptr;   // [K][img_i8_len] int8-digit parameter images (estep_i8.h), variant kEstepI8 only
    double* pivot_i8 = nullptr;        // [D] the pivot those images (and the sample digits) are centred on
    unsigned char* img_i8b = nullptr;  // [K][img_i8b_len] 3-digit images of the pruned E-step's bound pass
    gmmvb::BoundLevel bound;           // output blocks the int8 bound pass evaluates, and what the last passes at each level left (pass_plan.h)
    // carrying the E-step over a parameter update (gmmvb_set_drift, records.h): gamma / delta / Gamma of the pending
    // update, whether the records belong to the parameters of the last E-step on `bounds_rows` rows of `bounds_x`
    double* drift = nullptr;           // [4][K]: gamma, delta, c of the last E-step, Gamma
    bool have_drift = false;
    double typical_gamma = -1.0;       // mean gamma of the pending update if the caller knew it (<= 0: unknown)
    bool params_used = false;          // the parameters in force were the ones of the last E-step
    int64_t bounds_rows = 0;           // rows / matrix the records (and the ln rho array) belong to (0: nothing to carry)
    const void* bounds_x = nullptr;
    int64_t bounds_ldx = 0;
    int prev_pass = 0;                 // last E-step: 0 dense, 1 bound pass, 2 carried records, 3 dense sweep
    // per-row candidate records (records.h), allocated with the sample lists
    unsigned short* rec_k = nullptr;   // [8][npad]
    float* rec_d = nullptr;            // [8][npad]
    float* rec_B = nullptr;            // [npad]
    unsigned char* rec_exact = nullptr, *rec_sel = nullptr, *rec_flags = nullptr;   // [npad] each
    bool rec_valid = false;            // the records describe the last E-step's parameters on bounds_rows rows
    bool rec_live = false;             // the last E-step lived on records (read-outs go through them)
    float* ub32 = nullptr;             // [K][npad] upper bound of ln rho for every pair (rounded up), what the sweeps carry
    bool dense_valid = false;          // EVERY entry of ub32 is a value / bound under the last E-step's parameters
    int sweeps = 0;                    // dense sweeps since the last bound / dense pass (their bounds erode: at most 8)
    int* plan = nullptr;               // [K + 1] gather chunk plan (device)
    int* plan_m = nullptr;             // [K + 2] chunk plan of the list M-step
    double* epart = nullptr;           // [ceil(npad / 256)] listed pairs per selection block
    double* opart = nullptr;           // [ceil(npad / 256)] overflow rows per selection block
    double* mpart = nullptr;           // [ceil(npad / 256)] rows whose best component changed, per selection block
    double moved_since_sort = 0.0;     // their sum over the passes since the rows were last regrouped
    bool pend_first_sorted = false;    // the E-step whose counters are in flight regrouped the rows
    // counters of an E-step: [0] active pairs (r >= 2^-80), [1] pairs evaluated exactly, [2] overflow rows,
    // [3] rows whose best component changed.
    // Written on the device at the end of every E-step and copied to pinned host memory behind an event; the NEXT
    // E-step / M-step reads whatever has arrived (policy decisions lag one pass, results never depend on them).
    // [4] settled rows (see below), [5] pairs in the M-step's lists.
    // [6] pairs the M-step accumulates, [7] pairs of the proof round (int8 two-sided bounds instead of f64 values).
    double* ctr = nullptr;             // [8] device
    double* ctr_host = nullptr;        // [8] pinned
    hipEvent_t ctr_ev = nullptr;
    bool ctr_pending = false;          // a copy is in flight ...
    int pend_mode = 0;                 // ... of an E-step of this mode over pend_rows rows
    int64_t pend_rows = 0;
    double pend_round0 = 0.0;          // pairs that E-step evaluated before its counted selection round
    bool sweep_prev = false;           // the last sweep's first round used the previous pass's M-step lists
    // lag = counters of this rank's most recent E-step whose copy has arrived: what gmmvb_last_work reports, and the
    // policy's input in a single process.  pol = the same summed over the ranks of a row-sharded job
    // (gmmvb_policy_export / all-reduce / gmmvb_policy_import): once gmmvb_set_shard has been called the policy reads
    // nothing else that differs between ranks, so every rank takes the same decisions.
    gmmvb_pass_counters lag, pol;
    // unit costs and thresholds of the pass policy at this workspace's shape (policy.h); calibration from its own first
    // dense E-step / dense M-step / bound pass: HIP events around those launches, taken over when they have completed
    gmmvb::PolicyTable pt;
    // (opt_calibrate: also gmmvb_policy_calibrate(ws, 0))
    hipEvent_t cal_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};     // begin / end for dense E, dense M, bound pass
    double cal_pairs[3] = {0.0, 0.0, 0.0};       // pairs behind a pending measurement (0: none pending, -1: done)
    int cal_tries[3] = {0, 0, 0};                // measurements discarded so far
    bool sharded = false;              // gmmvb_set_shard: this workspace holds one shard of shard_rows rows over shard_ranks ranks
    int64_t shard_rows = 0;
    int shard_ranks = 1;
    double* pol_host = nullptr;        // [GMMVB_POLICY_LEN] pinned: the imported (summed) counters
    hipEvent_t pol_ev = nullptr;
    bool pol_pending = false;          // an import is in flight ...
    int pol_mode = 0;                  // ... of a pass of this mode
    bool pol_first_sorted = false;
    bool exp_counted = false;          // the last E-step counted its pairs (what gmmvb_policy_export may hand out)
    bool forget = false;               // gmmvb_forget: the next parameters are unrelated to the last E-step's
    double spare_last = -1.0;          // spare candidates per pair of the last pruned pass (diagnostics)
    double bound_fail_act = -1.0;      // active share of the pairs when a bound pass last left most of them candidates (< 0: never)
    double* cvec = nullptr;    // [K]
    double* pivot = nullptr;   // [D]
    double* dpart = nullptr;   // [ceil(npad / 1024)][K] block maxima of ln r (row_lse_kernel)
    double* thr = nullptr;     // [K] M-step skip thresholds: max_n ln r_nk - 80 ln 2 (valid while e_state == 1)
    double* apart = nullptr;   // [ceil(npad / 256)] pairs with ln r >= -80 ln 2 per selection block
    int64_t act_rows = 0;      // rows of the E-step whose active pairs were counted (0 = not counted)
    double act_host = -1.0;    // host copy of ctr[0] for that E-step (-1 = not fetched yet)
    double evaluated = 0.0;    // pairs the last E-step evaluated exactly (-1: on the device, see gmmvb_last_sparsity)
    // pruned E-step (estep.h): `prune` 0 never | 2 always | 1: when the previous E-step over the same rows left at most half
    // of the pairs relevant and N K >= 2^23
    int* lists = nullptr;      // [K][npad] sample lists (E-step candidates, then the M-step's active rows)
    bool active_lists = false; // the lists currently hold the active rows of the last E-step (scan + fill done)
    bool blk_fresh = false;    // blk still holds the block COUNTS of masks (not yet scanned into bases)
    int* khat = nullptr;       // [npad]
    int* counts = nullptr;     // [K]
    int* blk = nullptr;        // [blocks of 256 rows][K] candidates per selection block -> block bases (aux_kernels.h: blk_at)
    int* scan_parts = nullptr; // [K][kScanParts] partial sums of the scan over blk
    unsigned long long* masks = nullptr;   // [ceil(K / 64)][npad] candidate components of every sample
    double* slabs = nullptr;   // [S_cap][K][slab_len]
    // Settled rows (records.h): a row with ONE active component has r = 1.0 exactly, its addend to that component's
    // statistics does not depend on the parameters.  While the carried bounds prove that it stays so, the row is neither
    // evaluated (E) nor accumulated (M): its addend lives in `cache` (same layout as the statistics), which changes only
    // through the rows that settle or come loose in a pass (the M-step's delta lists).
    unsigned char* lock = nullptr;     // [npad] 0 free, 1 settled, 2 came loose in this pass, 3 settled in this pass
    unsigned char* lcomp = nullptr;    // [npad] cached rows: the component whose cache holds the row (K <= 256)
    float* dlock = nullptr;            // [npad] settled rows: upper bound of the whitened distance to their component
    float* rthr = nullptr;             // [npad] relevance threshold of the selection round (best exact value - 80 ln 2)
    unsigned long long* exit_ctr = nullptr;    // [4] device: candidate pairs of the pass that took the gather's early way out;
                                               //     (tile, component) columns the lazy sweep opened; pairs the table of
                                               //     project.h took off the proof lists (stateless sweep: pairs it left);
                                               //     tiles the sweep left without a loose row | tiles rec_finish_kernel
                                               //     skipped << 32 (GMMVB_DEBUG=2 only)
    unsigned long long* exit_host = nullptr;   // [4] pinned mirror (copied with the other counters)
    bool pend_lazy = false;                    // the pass behind the pending counters was a lazy sweep
    unsigned long long* dmask = nullptr;   // [ceil(K / 64)][npad] rows entering / leaving the cache in this pass
    int* dblk = nullptr;               // [blocks][K] their block counts
    unsigned long long* mmask = nullptr;   // [ceil(K / 64)][npad] the M-step's lists: active pairs of the rows not in the cache
    int* mblk = nullptr;               // [blocks][K] their block counts
    double* cache = nullptr;           // [stats_len] statistics of the settled rows
    double* spart = nullptr, *gpart = nullptr, *qpart = nullptr;   // [blocks] settled rows / listed pairs / M-step pairs per selection block
    unsigned long long* rmask = nullptr;   // read-outs of settled rows: their (row, component) pairs ...
    int* rblk = nullptr;                   // ... and block counts (allocated with the lists)
    bool lock_live = false;            // some rows may be settled: the list M-step must add the cache
    bool delta_pending = false;        // an E-step marked rows 2 / 3 / 4 and no M-step has applied them yet
    bool mlists_done = false;          // the lists hold the M-step's own lists (mmask) of the last E-step
    bool mlists_lost = false;          // ... did, until a read-out of settled rows used the buffers
    bool skip_used = false;            // some pass since the cache was last emptied was allowed to settle rows
    bool lock_reset = false;           // the settled state belongs to something else now: drop it at the next E-step
    bool settled_fresh = false;        // read-outs: the settled rows' ln rho / lse were re-evaluated for the parameters in force
    // (settle_margin: nats of slack demanded before a row is settled - < 0: never; 1e300: every single-component row)
    // Proof round (estep_i8.h, records.h): the three int8 digit planes of every row, in the internal row order, made with
    // the centred copy (gmmvb_prepare_rows) and again when the rows are regrouped.  Valid for the matrix xq_src while the
    // pivot they are centred on is the one the component images were packed for (xq_gen == img_gen).
    unsigned char* xq = nullptr;       // [npad][3][32 ceil(D / 32)]
    signed char* xqe = nullptr;        // [npad] exponent of the row's largest |x - pivot| (127: no digits)
    const void* xq_src = nullptr;
    int64_t xq_rows = 0, xq_ldx = 0;
    int pivot_gen = 0, xq_gen = -1, img_gen = -2;
    // The stateless sweep (project.h): bounds from the parameters in force and the rows' int8 digit planes instead of the
    // carried per-pair array.  gimg / gconst are made by gmmvb_set_params when a sweep can follow (regrouped rows, digit
    // planes about the pivot in force, a drift hint for the settled rows' own bound), tile_ref by the regrouping.
    unsigned char* gimg = nullptr;     // [K][proj_image_bytes] int8 digit images of g_jk, per reference component j
    void* gconst = nullptr;            // [K][32 proj_kblocks] float4 constants per (reference, column)
    int* tile_ref = nullptr;           // [blocks] reference component of every tile of kSelRows rows (regrouped order)
    bool proj_table = false;           // gimg / gconst describe the parameters in force
    bool tile_ref_valid = false;       // tile_ref describes the row order in force
    bool pend_proj = false;            // the pass behind the pending counters used the table (exit_ctr[1]: pairs it left / removed)
    float4* tmeta = nullptr;           // [blocks][K] the lazy sweep's state per tile and component (records.h)
    bool tmeta_valid = false;          // it describes the bound array as it is (only sweeps have written to it since)
    // Tile state of the settled rows (records.h), two ints per selection block of kSelRows rows:
    //   tile_loose[b]  valid rows of the tile whose flag is not 4 in the pass in flight: written by the PREV forms of
    //                  rec_sweep_kernel, lowered by rec_proof_decide_kernel by the rows it returns to flag 4;
    //   tile_quiet[b]  1 if tile_loose[b] was 0 when rec_finish_kernel last went over the tile.
    // While quiet_valid holds, a tile with tile_quiet == 1 is as that visit left it: every valid row has lock == 1; its rows
    // of masks, mmask and dmask are zero; khat, lcomp and lse are not due a write.  On these rest the shortcuts of
    // rec_finish_kernel (a tile quiet then and now: the per-block constants only) and settled_mask_kernel (own round: lcomp
    // only).  Set at the end of run_candidates of a sweep that counted (not the projected / filtered form); cleared - like
    // tmeta_valid: when in doubt - by every E-step before its first launch (so by dense and bound passes and the
    // regrouping), by a cache reset, and by whatever else touches those arrays or the row order: load_r, yield_scratch, a
    // new matrix or pivot, gmmvb_forget, the diagnostic proof.  (The read-out of settled rows writes lse, ln rho entries
    // and the read-out lists only: the state stands.)
    // The two arrays live in perm_tmp, which is idle between regroupings (a regrouping voids the state anyway): the
    // workspace's buffer list and its byte count stay what they were.  A workspace that shares its scratch with other tiles
    // loses it to them before every pass of its own - the state would never be valid - and keeps none.
    bool quiet_valid = false;
    bool pend_quiet = false;           // the pass behind the pending counters counted its quiet tiles (exit_ctr[3])
    double lag_quiet = -1.0;           // ... and their number once the copy has arrived (< 0: not counted; GMMVB_DEBUG=2)
    double lag_skipped = -1.0;         // ... and the tiles rec_finish_kernel took the short way through (the counter's upper half)
    int* tile_loose() const { return (opt_quiet_tiles && perm_tmp && !(scratch && scratch->refs > 1)) ? perm_tmp : nullptr; }
    int* tile_quiet() const { return tile_loose() ? perm_tmp + (npad + 255) / 256 : nullptr; }
    double* ppart = nullptr;           // [blocks] pairs of the proof round per selection block
    // rows grouped by dominant component (aux_kernels.h): internal row i = the caller's row perm[i]
    void* xp = nullptr;        // [max_rows][D] x in internal row order (storage dtype), allocated with the lists
    int* perm = nullptr, *iperm = nullptr, *perm_tmp = nullptr;   // [npad] each
    bool sorted = false;       // xp / perm / iperm are in force for the matrix xc_src (else the internal order is the caller's)
    int64_t sorts = 0;         // regroupings since the workspace was created
    double* xc = nullptr;      // [npad][16T] centred f64 copy of the sample matrix (M-step operand), optional
    const void* xc_src = nullptr;   // the x it was made from (null = not prepared)
    int64_t xc_rows = 0, xc_ldx = 0;
    bool xc_stale = false;     // the rows were regrouped since xc was made: it is rebuilt from xp when a kernel needs it
    // c_degree > 128 (generic.h): plain f64 kernels on the raw parameters, no images, no lists
    double* gen_u = nullptr;           // [K][D][D]
    double* gen_m = nullptr;           // [K][D]
    double* gen_first = nullptr;       // [gen_S][K][D + 2] partial ns, h, a per row split
    double* gen_second = nullptr;      // [gen_S][K][tri_pairs(T)][256] partial B tiles per row split
    gmmvb::BufferPlan buffers;         // every device / pinned buffer above, as created (workspace_plan.h); bytes = their sum
    int64_t bytes = 0;
    bool have_params = false;
    int e_state = 0;           // 0 none, 1 E-step output, 2 responsibilities loaded directly, 3 HMM gamma,
                               // 4 emission as rho' / mx in the HMM state, no ln rho array (hmmvb_emission_target)
    int64_t e_rows = 0;
    char info[512] = {0};
    hipError_t hip_err = hipSuccess;   // first failed event record / counter reset of the pass in flight (capi.hip: note_hip)
    // launches since the workspace was created (gmmvb_pass_counts): E dense, E bound pass, E carried bounds,
    // pruned E-step that fell back to the dense kernel, E sweep of carried bounds, M dense, M lists,
    // candidate gathers
    int64_t passes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool prof = false;
    bool prof_light = false;           // gmmvb_profile_enable(ws, 2): only the spans of the groups that can dominate a step
    bool span_open = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // E begin/end, M begin/end
    bool ev_e = false, ev_m = false;
    // per-kernel-group spans of the last E-step + M-step (gmmvb_profile_spans): slot, begin/end event
    static constexpr int kMaxSpans = 24;
    int n_spans = 0;
    int span_slot[kMaxSpans] = {0};
    hipEvent_t span_ev[2 * kMaxSpans] = {nullptr};
    gmmvb_hmm_state* hmm = nullptr;
    bool hmm_skip_h = false;           // hmmvb_skip_h: the M-step of an HMM pass leaves h = 0 (and does not read the ln rho array)
    bool hmm_no_lnrho = false;         // the last E-step handed its emission to the HMM state (e_state 4, then 3): no ln rho array
    bool lse_stale = false;            // the last dense E-step of an HMM workspace did not make lse (only a read-out wants it)
};

namespace gmmvb {
// a developer switch (workspace_plan.h): looked at only when GMMVB_DEBUG is set
inline const char* dev_env(const char* name) { return dev_switch(std::getenv, name); }
int fail(int code, const char* what, hipError_t e = hipSuccess);     // sets the thread-local message
void hmm_state_destroy(gmmvb_hmm_state* h);
const double* hmm_gamma_cm(const gmmvb_hmm_state* h);                 // [K][npad] responsibilities of the last pass (after hmm_ensure_gamma_cm)
const double* hmm_gamma_tm(const gmmvb_hmm_state* h);                 // [npad][Kp] the same, time-major in lane order (hmm.h)
int hmm_padded_states(const gmmvb_hmm_state* h);                      // Kp
bool hmm_fused_emission(const gmmvb_hmm_state* h);                    // gmmvb_estep hands rho' / mx straight to the HMM state (e_state 4)
hipError_t hmm_ensure_gamma_cm(gmmvb_hmm_state* h, hipStream_t st);   // transposes gamma once per pass, on demand
}  // namespace gmmvb
