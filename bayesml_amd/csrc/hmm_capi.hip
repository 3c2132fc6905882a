// C ABI of the HMM forward-backward pass (include/gmmvb.h, hmmvb_* entry points).
#include "workspace.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <new>
#include <type_traits>

#include "hmm.h"
#include "launch.h"
#include "hmm_generic.h"
#include "hmm_wide.h"

#include <cstdlib>

using namespace gmmvb;

namespace {

constexpr int kLncBlocks = 1024;
constexpr int kHmmCheckBlocks = 1024;      // grid of hmm_boundary_check_kernel (grid-stride over 40 MB of boundary vectors at config 5: 64 blocks took 0.08 ms)
// the forgetting pass stands if no entry of a (sum-1 normalised) boundary vector moves by more than this RELATIVE to itself
// when its chunk is started from the sweep's vector instead of the uniform one (hmm.h, hmm_boundary_check_kernel<true>: a test
// in the Hilbert metric, in which the recursion is non-expansive): a fully forgotten start leaves the rounding noise of sums
// of positive terms, a few 1e-16 relative per entry whatever its size
constexpr double kHmmForgetTol = 2e-13;
// the Viterbi pass's coalescence test (absolute, nats, on omega - max of a chunk's end vector): the two replays of a chunk
// round sums that reach ~1e4 in magnitude inside the chunk (ulp 2e-12) differently, so ~1e-11 is the noise; start-vector
// errors add up to at most chunks x tol over the sequence (max-plus maps are 1-Lipschitz): 8e-6 nats at 4e4 chunks, below
// the rounding of the sequential recursion's own sums at that length (scores ~5e8: ulp 6e-8 per step)
constexpr double kVitCoalesceTol = 2e-10;
constexpr int64_t kHmmGenericChunk = 256;      // more than 128 states: steps per workgroup in the forgetting pass
// 65 .. 128 states, long sequences: chunk products / boundary pass / replays of hmm_wide.h between the generic prep and xi-sum
constexpr int64_t kHmmWideChunk = 256;
constexpr int64_t kHmmWideMinSteps = 2048;        // (shorter sequences: the sequential kernels - a handful of chunks fills nothing)
// Long sequences (more than kHmmLongFrom steps): chunks of 256 steps and a two-level boundary pass (hmm.h, H3a / H3b).
// (round 4: from 2^15 steps instead of 2^18 - with the forgetting pass the long-sequence form costs two sweeps instead of the chunk
// products, and its short chunks shorten the replays' chains of dependent steps: T = 2e5 4.1 ms per iteration against 1.5)
constexpr int64_t kHmmLongFrom = int64_t(1) << 15;
constexpr int64_t kHmmShortForgetFrom = 4096;      // from here to kHmmLongFrom: the forgetting pass on chunks of kHmmShortChunk steps
constexpr int64_t kHmmShortChunk = 32;

// f(std::integral_constant<int, KT>) for the KT in Lo .. Hi that kt names (KT: 16-state blocks, the kernels' template
// argument); any other kt takes Hi
template <int Lo, int Hi, typename F>
auto dispatch_kt(int kt, F&& f) {
    if constexpr (Lo < Hi) {
        if (kt == Lo) return f(std::integral_constant<int, Lo>{});
        return dispatch_kt<Lo + 1, Hi>(kt, f);
    } else {
        return f(std::integral_constant<int, Hi>{});
    }
}

}  // namespace

struct gmmvb_hmm_state {
    int K = 0, Kp = 0, KT = 0;
    int64_t npad = 0, max_chunks = 0, xi_waves = 0;
    double* rho_tm = nullptr;     // [npad][Kp] lane order
    double* alpha_tm = nullptr;   // [npad][Kp]
    double* gamma_tm = nullptr;   // [npad][Kp]
    double* w_tm = nullptr;       // [npad][Kp]
    double* gamma_cm = nullptr;   // [K][npad]  component-major copy of gamma, made on demand (hmm_ensure_gamma_cm): read-outs and
                                  //            the M-step kernels of D > 16; the D <= 16 M-step reads gamma_tm itself
    bool gamma_cm_valid = false;
    int64_t gamma_rows = 0;       // rows of the last forward-backward pass
    double* mx = nullptr;         // [npad]
    double* cprime = nullptr;     // [npad]
    double* prod = nullptr;       // [max_chunks][Kp][Kp]
    double* prod_t = nullptr;     // [max_chunks][Kp][Kp] their transposes (65 .. 128 states: the backward boundary pass reads them)
    double* qprod_t = nullptr;    // [max_chunks / kHmmSuper + 2][Kp][Kp] transposes of the super-chunk products (65 .. 128 states)
    double* fstart = nullptr;     // [max_chunks][Kp]
    double* bend = nullptr;       // [max_chunks][Kp]
    double* qprod = nullptr;      // [max_chunks / kHmmSuper + 2][Kp][Kp] super-chunk products (two-level boundary pass)
    double* fstart_s = nullptr, *bend_s = nullptr;   // [max_chunks / kHmmSuper + 2][Kp] their boundary vectors
    double* xi_slabs = nullptr;   // [xi_waves][Kp][Kp]
    double* lnc_partial = nullptr;   // [kLncBlocks]
    unsigned char* phi = nullptr; // [npad][Kp] Viterbi back-pointers (allocated on first use by hmmvb_enable)
    int* last_state = nullptr;
    // more than 64 states: the sequential kernels of hmm_generic.h; 65 .. 128 states and long sequences: the chunk-parallel
    // kernels of hmm_wide.h for the forward-backward pass (generic stays set: prep, xi-sum, Viterbi are the generic ones)
    bool generic = false;
    bool wide = false;
    double* a_t = nullptr;        // [K][K] transpose of A~
    unsigned short* phi16 = nullptr;   // [npad][K] back-pointers, natural order
    int64_t bytes = 0;
    int64_t vec_chunks = 0;       // rows of fstart / bend / fstart2 / bend2
    int64_t xi_slab_cap = 0;      // slabs xi_slabs has room for
    bool xi_separate = false;     // developer switch GMMVB_HMM_XI_SEPARATE: hmm_xi_sum_kernel as in round 3
    bool w_valid = false;         // the last pass wrote w_tm (false: the backward replay summed xi itself, hmm.h H5 XI)
    double* fstart2 = nullptr, *bend2 = nullptr;   // [max_chunks][Kp] the replays' own boundary vectors (forgetting pass)
    int* gate_dev = nullptr;      // 1: the forgetting pass's vectors do not stand, the products path runs
    int* gate_host = nullptr;     // pinned copy, read when the next call begins
    hipEvent_t gate_ev = nullptr;
    bool gate_pending = false, spec_on = true;
    bool vit_coalesced = false;   // the last hmmvb_viterbi call ran the coalescence pass (its gate: gate_dev[1])
    int64_t sweep_len = 64;       // steps next to a chunk boundary the forgetting pass's first stage walks (run<KT>; 32 failed one pass in seven at config 5, 64 none)
    int64_t chunk_floor = 0;      // run<KT>: a pass that did not stand on chunks shorter than kHmmLongChunk doubles them for the next ones
    int64_t gate_l = 0;           // chunk length of the pass whose gates are pending
    int short_hold = 0, short_hold_len = 4;      // calls that skip the short first stage after it did not stand (4, 8 ... 64 while it keeps failing)
    bool gate_two_stage = false;  // the pass whose gates are pending had a short first stage
    int spec_hold = 0, spec_hold_len = 8, last_gate = -1;   // last_gate: -1 no forgetting pass, 0 it stood, 1 products path behind it
    bool fuse_emission = false;   // hmmvb_emission_target: gmmvb_estep writes rho' / mx here (hmm.h H0 + H1) and no ln rho array
};

namespace {
// Every f64 device buffer of the state with its length in elements (0: not used at this state count).  hmmvb_enable
// allocates from this table and hmm_state_destroy frees by it.
struct HmmBuf { double** p; int64_t n; };
std::array<HmmBuf, 20> hmm_buffers(gmmvb_hmm_state* h) {
    const int64_t tk = h->npad * h->Kp, kk = (int64_t)h->Kp * h->Kp, supers = h->max_chunks / kHmmSuper + 2;
    const int64_t vecs = h->vec_chunks * h->Kp;
    return {{{&h->rho_tm, tk}, {&h->alpha_tm, tk}, {&h->gamma_tm, tk}, {&h->w_tm, tk},
             {&h->gamma_cm, (int64_t)h->K * h->npad}, {&h->mx, h->npad}, {&h->cprime, h->npad},
             {&h->prod, h->max_chunks * kk}, {&h->fstart, vecs}, {&h->bend, vecs}, {&h->xi_slabs, h->xi_slab_cap * kk},
             {&h->lnc_partial, kLncBlocks},
             {&h->qprod, supers * kk}, {&h->fstart_s, supers * h->Kp}, {&h->bend_s, supers * h->Kp},
             {&h->a_t, h->generic ? (int64_t)h->K * h->K : 0},
             {&h->prod_t, h->wide ? h->max_chunks * kk : 0}, {&h->qprod_t, h->wide ? supers * kk : 0},
             {&h->fstart2, vecs}, {&h->bend2, vecs}}};
}
}  // namespace

namespace gmmvb {
void hmm_state_destroy(gmmvb_hmm_state* h) {
    if (!h) return;
    for (const HmmBuf& b : hmm_buffers(h))
        if (*b.p) (void)hipFree(*b.p);
    if (h->gate_dev) (void)hipFree(h->gate_dev);
    if (h->gate_host) (void)hipHostFree(h->gate_host);
    if (h->gate_ev) (void)hipEventDestroy(h->gate_ev);
    if (h->phi) (void)hipFree(h->phi);
    if (h->phi16) (void)hipFree(h->phi16);
    if (h->last_state) (void)hipFree(h->last_state);
    delete h;
}
const double* hmm_gamma_cm(const gmmvb_hmm_state* h) { return h ? h->gamma_cm : nullptr; }
const double* hmm_gamma_tm(const gmmvb_hmm_state* h) { return h ? h->gamma_tm : nullptr; }
int hmm_padded_states(const gmmvb_hmm_state* h) { return h ? h->Kp : 0; }
// the emission of one feature tile straight into rho' / mx (hmm_emission_mfma16_kernel): asked for, and a shape it covers
// (up to 32 states: beyond, a wave's K values per row no longer fit its registers beside the pipeline's operands)
bool hmm_fused_emission(const gmmvb_hmm_state* h) { return h && h->fuse_emission && !h->generic && h->KT <= 2; }
template <typename XT, bool V>
static void launch_emission16(gmmvb_hmm_state* h, unsigned grid, hipStream_t st, const EstepArgs& a) {
    dispatch_kt<1, 2>(h->KT, [&](auto kt) {
        hipLaunchKernelGGL((hmm_emission_mfma16_kernel<XT, V, decltype(kt)::value>), dim3(grid), dim3(256), 0, st,
                           static_cast<const XT*>(a.x), a.ldx, a.n_rows, a.D, a.img, a.cvec, a.K, h->rho_tm, h->mx);
    });
}
hipError_t hmm_launch_emission16(gmmvb_hmm_state* h, int x_is_f64, bool vec, hipStream_t st, const EstepArgs& a, const char** name) {
    const int64_t rows_per_wg = 4 * 16 * (h->KT == 1 ? 4 : 2);       // (hmm.h: NB row tiles per wave)
    const int64_t wgs = (a.n_rows + rows_per_wg - 1) / rows_per_wg;
    const unsigned grid = (unsigned)std::min<int64_t>(wgs, int64_t(1) << 20);
    *name = "hmm_emission_mfma16_kernel";
    if (x_is_f64) {
        if (vec) launch_emission16<double, true>(h, grid, st, a);
        else launch_emission16<double, false>(h, grid, st, a);
    } else {
        if (vec) launch_emission16<float, true>(h, grid, st, a);
        else launch_emission16<float, false>(h, grid, st, a);
    }
    return hipGetLastError();
}
// gamma component-major for whoever reads it that way: transposed once per forward-backward pass, and only if asked for
hipError_t hmm_ensure_gamma_cm(gmmvb_hmm_state* h, hipStream_t st) {
    if (!h || h->gamma_cm_valid || h->gamma_rows < 1) return hipSuccess;
    const int64_t T = h->gamma_rows;
    hipLaunchKernelGGL(hmm_gamma_to_cm_kernel, dim3((unsigned)((T + 63) / 64), (unsigned)((h->K + 63) / 64)), dim3(256), 0, st,
                       h->gamma_tm, T, h->K, h->Kp, h->npad, h->gamma_cm);
    h->gamma_cm_valid = true;
    return hipGetLastError();
}
}  // namespace gmmvb

namespace {

// ---- forward-backward: what the three state-count ranges share ------------------------------------------------------------
// The gate of the last forgetting pass, once its pinned copy has arrived: a pass that did not stand holds the next ones off -
// for 8 calls, then 16, ... 64 while it keeps failing (sticky chains with flat emissions pay for a sweep and a replay each time).
bool consume_gate(gmmvb_hmm_state* h, bool wait) {
    if (!h->gate_pending) return true;
    const hipError_t e = wait ? hipEventSynchronize(h->gate_ev) : hipEventQuery(h->gate_ev);
    if (e == hipErrorNotReady) return true;
    if (e != hipSuccess) return false;
    h->gate_pending = false;
    h->last_gate = h->gate_host[0];
    if (h->gate_two_stage) {
        // the first stage's sweeps walked only the steps next to the boundaries: when that was not enough the whole-chunk
        // stage behind its gate has done the work (a sweep and two replays more): go straight to whole chunks for a while
        if (h->gate_host[1] != 0) {
            h->short_hold = h->short_hold_len;
            h->short_hold_len = std::min(64, 2 * h->short_hold_len);
        } else {
            h->short_hold_len = 4;
        }
    }
    if (h->last_gate != 0 && h->gate_l > 0 && h->gate_l < kHmmLongChunk) {
        // the chunks were shorter than the recursions' memory: longer ones at once (no hold-off - that is for sequences
        // whose 256-step chunks do not stand either)
        h->chunk_floor = 2 * h->gate_l;
    } else if (h->last_gate != 0) {
        h->spec_hold = h->spec_hold_len;
        h->spec_hold_len = std::min(64, 2 * h->spec_hold_len);
    } else {
        h->spec_hold_len = 8;
    }
    h->gate_l = 0;
    return true;
}

// May this call try the forgetting pass?  Not on a shape or a state that does not take it (`eligible`), and not while a pass
// that did not stand holds the next ones off (consume_gate): such a call counts the hold down.
// (a gate copy still in flight - a caller that does not synchronise between calls - only means the last outcome is not known yet)
bool may_try_forgetting(gmmvb_hmm_state* h, bool eligible) {
    if (!eligible || !h->spec_on || h->gate_dev == nullptr) return false;
    if (h->spec_hold > 0) {
        --h->spec_hold;
        return false;
    }
    return true;
}

// One restart test, the core of the forgetting pass below and of the Viterbi pass's coalescence pass: sweep() walks every
// chunk from a blank start and leaves the chunks' end vectors in f / b, replay() runs every chunk from its neighbour's end
// vector and leaves its own in f2 / b2; if an entry of the two sets differs by more than tol (Relative: relative to itself),
// the start vectors do not stand and the gate `opens`.  behind: the gate that must have opened for the test to run at all.
template <bool Relative, typename Sweep, typename Replay>
void restart_test(hipStream_t st, Sweep sweep, Replay replay, const double* f, const double* f2, const double* b, const double* b2,
                  int64_t n, int Kp, double tol, int* opens, const int* behind) {
    sweep();
    replay();
    hipLaunchKernelGGL(hmm_boundary_check_kernel<Relative>, dim3(kHmmCheckBlocks), dim3(256), 0, st, f, f2, b, b2, n, Kp, tol, opens,
                       behind);
}

// ---- the forgetting pass (round 4): chunk boundary vectors without the chunk products ------------------------------------
// The scaled recursions forget their start vector: started from the UNIFORM vector, a chunk of 256 steps of a sequence with
// informative emissions ends in the same normalised alpha (beta~) as from the true one - to rounding.  So: a sweep of both
// recursions over all chunks from uniform starts (K^2 per step, no stores) gives every chunk a start vector, the replays
// run from those, and their own end vectors are compared with the sweeps': the difference IS (to first order) the error
// of the start vectors used, and at <= 2e-13 RELATIVE per entry (kHmmForgetTol, a Hilbert-metric test) they stand.
// Otherwise - slow mixing, flat emissions - the gate opens and the path's exact form runs behind it (its kernels return at
// once while the gate is shut), replays included: the result depends on the forgetting only through start vectors proven
// within chunks x 4e-13 of the exact ones in the Hilbert metric.  Up to 128 states the exact form is the chunk products,
// T 2 K^3 flop (10 ms of f64 MFMA at config 5; 85 % of the iteration at 65 .. 128 states), beyond them ONE workgroup's walk of
// the whole sequence (seconds per million steps); the sweeps are two more passes of K^2 per step.  A call that needed the
// exact form holds the pass off for the next eight calls (the gate is copied to pinned memory and looked at when the next
// call begins: no synchronisation).
//
// The path gives its launches: sweeps(steps, behind) walks `steps` steps up to every chunk boundary from uniform starts
// into fstart / bend, replays(behind) runs from those into fstart2 / bend2, exact(gate) is the whole exact form (gate nullptr:
// unconditionally).  pi_tilde: the sequence's own start for hmm_alpha0_kernel (nullptr: the path's sweeps set it themselves).
// `staged` (up to 64 states): a first stage whose sweeps walk only the W < L steps next to every boundary (hmm.h,
// hmm_sweeps_kernel); if the replays' own boundary vectors agree, done.  Otherwise gate_a opens the second stage - whole-chunk
// sweeps, replays, check -, and only if that does not stand either gate_b opens the exact form.
template <typename Sweeps, typename Replays, typename Exact>
hipError_t forgetting_pass(gmmvb_hmm_state* h, hipStream_t st, bool attempt, const double* pi_tilde, int64_t n_chunks, int64_t L,
                           int64_t W, bool staged, Sweeps sweeps, Replays replays, Exact exact) {
    if (!attempt) {
        h->last_gate = -1;
        return exact(nullptr);
    }
    int* const gate_b = h->gate_dev;           // opens the exact form
    int* const gate_a = h->gate_dev + 2;       // opens the whole-chunk stage ([1] is the Viterbi pass's)
    if (hipError_t eg = hipMemsetAsync(gate_b, 0, sizeof(int), st); eg != hipSuccess) return eg;      // (the gates must be shut before the checks)
    if (staged) {
        if (hipError_t eg = hipMemsetAsync(gate_a, 0, sizeof(int), st); eg != hipSuccess) return eg;
        h->gate_two_stage = W < L;
        h->gate_l = L;
    }
    if (pi_tilde)
        hipLaunchKernelGGL(hmm_alpha0_kernel, dim3(1), dim3(256), 0, st, h->rho_tm, pi_tilde, h->K, h->Kp, n_chunks, h->fstart,
                           h->bend, h->cprime);
    auto stage = [&](int64_t steps, int* opens, const int* behind) {
        restart_test<true>(st, [&] { sweeps(steps, behind); }, [&] { replays(behind); }, h->fstart, h->fstart2, h->bend, h->bend2,
                           (n_chunks - 1) * h->Kp, h->Kp, kHmmForgetTol, opens, behind);
    };
    if (W < L) stage(W, gate_a, nullptr);
    stage(L, gate_b, W < L ? gate_a : nullptr);
    // (the pinned copies only steer the NEXT calls - hold the pass off after one that needed the exact form, the short stage
    // after one that needed whole chunks; if they cannot be made, the next calls simply try again)
    h->gate_pending = hipMemcpyAsync(h->gate_host, gate_b, sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess &&
                      (!staged || hipMemcpyAsync(h->gate_host + 1, gate_a, sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess) &&
                      hipEventRecord(h->gate_ev, st) == hipSuccess;
    return exact(gate_b);
}

// The pass's tail: the partial sums of ln c, and hmm_finish_kernel turns them and the path's xi slabs into the results.
// w_valid: the pass wrote w_tm (false: the backward replay summed xi itself, hmm.h H5 XI).
hipError_t finish_pass(gmmvb_hmm_state* h, hipStream_t st, int64_t T, const double* a_tilde, int64_t n_slabs, bool w_valid,
                       double* out) {
    const int n_part = (int)std::min<int64_t>(kLncBlocks, (T + 255) / 256);
    hipLaunchKernelGGL(hmm_lnc_partial_kernel, dim3(n_part), dim3(256), 0, st, h->cprime, h->mx, T, h->lnc_partial);
    hipLaunchKernelGGL(hmm_finish_kernel, dim3((unsigned)((h->K * h->K + 7) / 8)), dim3(256), 0, st, h->xi_slabs, n_slabs, a_tilde,
                       h->K, h->Kp, h->lnc_partial, n_part, T, h->gamma_tm, out);
    h->w_valid = w_valid;
    h->gamma_cm_valid = false;                 // (made on demand: hmm_ensure_gamma_cm)
    h->gamma_rows = T;
    return hipGetLastError();
}

// ---- up to 64 states (hmm.h) ------------------------------------------------------------------------------------------------
// Chunk length of this call (read before may_try_forgetting counts a hold down).
int64_t narrow_chunk_len(int64_t T, int num_cu, const gmmvb_hmm_state* h) {
    if (T > kHmmLongFrom) {
        int64_t L = kHmmLongChunk;
        // long sequences whose 256-step chunks are few (64 to a replay workgroup, and the replays / sweeps are chains of
        // dependent steps whose length is the chunk's): chunks of 128 steps - twice the waves, half the chain
        // (config 5 shape on one box: T = 4e5 2.64 -> 2.12 ms per iteration, 1e6 3.21 -> 2.61, 3e6 4.85 -> 4.56; at 8e6 the shorter
        // chunks lose, 9.79 -> 10.16: the limit is a replay workgroup per CU)
        // (round 5: down to 32 steps - with the products behind the gates a chunk only has to be long enough for the recursions to
        // forget their start, and the replays are chains of dependent steps: T = 1e5 ran 128-step chains on 13 workgroups)
        // ... and up again, for good, when a pass on short chunks did not stand (chunk_floor; consume_gate)
        while (L > kHmmShortChunk && L > h->chunk_floor && (T - 1 + L - 1) / L < 64 * (int64_t)num_cu) L /= 2;
        return L;
    }
    // Short sequences (round 5): the one-level products path balances a sequential pass over T / L chunk products against
    // replay chains of L steps (T = 1e4: L = 64, 157 products one after the other - 0.25 ms - and two 64-step chains); with the
    // chunk start vectors from the forgetting pass the chunks can be short - 32 steps: a 32-step sweep and two 32-step replay
    // chains - and the products only run behind the gate.  While a failed gate holds the pass off, the formula's chunks.
    if (T >= kHmmShortForgetFrom && h->spec_on && h->gate_dev != nullptr && h->spec_hold == 0)
        return std::min<int64_t>(kHmmLongChunk, std::max<int64_t>(kHmmShortChunk, h->chunk_floor));
    // the products path's balance of the sequential boundary scan (T/L steps of ~1.5 us) against the replay depth (L steps of
    // ~4 us forward+backward): L ~ sqrt(T * 1.5 / 4), a power of two in [16, 4096]
    int64_t L = 16;
    while (L < 4096 && 8 * L * L < 3 * T) L *= 2;
    return L;
}

template <int KT>
hipError_t run(gmmvb_workspace* ws, gmmvb_hmm_state* h, int64_t T, const double* pi_tilde, const double* a_tilde,
               double* out, hipStream_t st) {
    const int K = h->K, Kp = h->Kp;
    const int64_t L = narrow_chunk_len(T, ws->num_cu, h);
    const bool long_seq = T > kHmmLongFrom;
    const int64_t n_chunks = T > 1 ? (T - 1 + L - 1) / L : 0;
    if (ws->e_state != 4)          // (4: the emission kernel has written rho' and mx itself)
        hipLaunchKernelGGL(hmm_prep_kernel, dim3((unsigned)((T + kPrepSteps - 1) / kPrepSteps)), dim3(256),
                           ((size_t)Kp * (kPrepSteps + 1) + kPrepSteps) * sizeof(double), st, ws->lnrho, ws->npad, T, K, Kp, h->rho_tm,
                           h->mx);
    const bool two_level = long_seq && n_chunks > 2 * kHmmSuper;
    const unsigned grid = (unsigned)((n_chunks + 4 * kReplayChunks - 1) / (4 * kReplayChunks));      // kReplayChunks chunks per wave, 4 waves per block
    // the xi sum inside the backward replay (one slab per replay wave) unless the slabs do not fit / developer switch
    // (up to 32 states: with three or four 16-state blocks the accumulators no longer fit beside the operator's registers)
    const bool xi_fused = KT <= 2 && n_chunks > 0 && kReplayChunks == 16 && (int64_t)grid * 4 <= h->xi_slab_cap && !h->xi_separate;
    auto replays = [&](const double* fs, const double* be, double* f_out, double* b_out, const int* gate) {
        hipLaunchKernelGGL((hmm_forward_replay_kernel<KT>), dim3(grid), dim3(256), 0, st, h->rho_tm, a_tilde, K, T, L, n_chunks, fs,
                           h->alpha_tm, h->cprime, 0, f_out, gate);
        if constexpr (KT <= 2 && kReplayChunks == 16) {
            if (xi_fused)
                hipLaunchKernelGGL((hmm_backward_replay_kernel<KT, true>), dim3(grid), dim3(256), 0, st, h->rho_tm, a_tilde, K, T, L,
                                   n_chunks, be, h->alpha_tm, h->cprime, h->gamma_tm, h->w_tm, h->xi_slabs, b_out, gate);
        }
        if (!xi_fused)
            hipLaunchKernelGGL((hmm_backward_replay_kernel<KT, false>), dim3(grid), dim3(256), 0, st, h->rho_tm, a_tilde, K, T, L,
                               n_chunks, be, h->alpha_tm, h->cprime, h->gamma_tm, h->w_tm, nullptr, b_out, gate);
    };
    auto sweeps = [&](int64_t steps, const int* behind) {
        hipLaunchKernelGGL((hmm_sweeps_kernel<KT>), dim3(grid, 2), dim3(256), 0, st, h->rho_tm, a_tilde, K, T, L, n_chunks, h->fstart,
                           h->bend, steps, behind);
    };
    auto products_path = [&](const int* gate) {
        if (n_chunks > 0)
            hipLaunchKernelGGL((hmm_chunk_products_kernel<KT>), dim3((unsigned)((n_chunks + 3) / 4)), dim3(256), 0, st, h->rho_tm,
                               a_tilde, K, T, L, n_chunks, h->prod, gate);
        if (two_level) {
            const int64_t n_super = (n_chunks + kHmmSuper - 1) / kHmmSuper;
            hipLaunchKernelGGL((hmm_super_products_kernel<KT>), dim3((unsigned)n_super), dim3(256), 0, st, h->prod, n_chunks, h->qprod,
                               gate);
            hipLaunchKernelGGL((hmm_boundary_scan_kernel<KT>), dim3(1), dim3(128), 0, st, h->rho_tm, pi_tilde, h->qprod, K, n_super,
                               h->fstart_s, h->bend_s, h->cprime, h->alpha_tm, h->gamma_tm, h->w_tm, gate);
            hipLaunchKernelGGL((hmm_boundary_fill_kernel<KT>), dim3((unsigned)n_super), dim3(128), 0, st, h->prod, n_chunks,
                               h->fstart_s, h->bend_s, h->fstart, h->bend, gate);
        } else {
            hipLaunchKernelGGL((hmm_boundary_scan_kernel<KT>), dim3(1), dim3(128), 0, st, h->rho_tm, pi_tilde, h->prod, K, n_chunks,
                               h->fstart, h->bend, h->cprime, h->alpha_tm, h->gamma_tm, h->w_tm, gate);
        }
        if (n_chunks > 0) replays(h->fstart, h->bend, nullptr, nullptr, gate);
        return hipSuccess;
    };
    const bool attempt = may_try_forgetting(h, two_level || (!long_seq && T >= kHmmShortForgetFrom));
    // the first stage's sweeps walk sweep_len steps, unless whole chunks are no longer or a failed first stage holds it off
    int64_t W = std::min<int64_t>(L, h->sweep_len);
    if (attempt && W < L && h->short_hold > 0) {
        --h->short_hold;
        W = L;
    }
    const hipError_t e = forgetting_pass(h, st, attempt, pi_tilde, n_chunks, L, W, /*staged=*/true, sweeps,
                                         [&](const int* behind) { replays(h->fstart, h->bend, h->fstart2, h->bend2, behind); },
                                         products_path);
    if (e != hipSuccess) return e;
    // xi sum over t = 1 .. T-1
    int64_t n_waves = h->xi_waves;
    int64_t steps = T > 1 ? round_up((T - 1 + n_waves - 1) / n_waves, 4) : 4;
    n_waves = T > 1 && !xi_fused ? (T - 1 + steps - 1) / steps : 0;
    if (n_waves > 0)
        hipLaunchKernelGGL((hmm_xi_sum_kernel<KT>), dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0, st, h->alpha_tm, h->w_tm, T,
                           steps, h->xi_slabs);
    // waves of the last block beyond n_waves write slabs too (zeros): include them only if they exist
    const int64_t n_slabs = xi_fused ? (int64_t)grid * 4 : (n_waves > 0 ? ((n_waves + 3) / 4) * 4 : 0);
    return finish_pass(h, st, T, a_tilde, n_slabs, /*w_valid=*/!xi_fused, out);
}

// the kernels of hmm_generic.h and hmm_wide.h ask for more than 48 KB of dynamic LDS at some state counts
template <typename Kern>
hipError_t seq_lds(Kern kern, size_t bytes) {
    return bytes > 48 * 1024 ? hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)bytes)
                             : hipSuccess;
}

// ---- 65 .. 128 states, at least kHmmWideMinSteps steps (hmm_wide.h between the generic prep and the wide xi sum) -----------
template <int KT>
hipError_t run_wide(gmmvb_workspace* ws, gmmvb_hmm_state* h, int64_t T, const double* pi_tilde, const double* a_tilde,
                    double* out, hipStream_t st) {
    const int K = h->K, Kp = h->Kp;
    // chunks of 256 steps, 64 to a replay workgroup (one per CU: the A fragments fill its LDS) - or of 128 steps while that leaves
    // CUs without a workgroup (T = 2e6: 123 workgroups of 256-step chunks on 256 CUs; the replays and sweeps are chains of
    // dependent steps, twice the workgroups halve them; chunks of 64 steps were too short for the forgetting pass at K = 128, D = 8)
    int64_t L = kHmmWideChunk;
    if ((T - 1 + L - 1) / L < 64 * (int64_t)ws->num_cu && (T - 1 + L / 2 - 1) / (L / 2) <= h->max_chunks) L /= 2;
    const int64_t n_chunks = (T - 1 + L - 1) / L;
    if (n_chunks > h->max_chunks) return hipErrorInvalidValue;
    const size_t fb = hmm_wide_frag_bytes<KT>();
    hipError_t e = seq_lds(hmm_chunk_products_wide_kernel<KT>, fb + 64);
    if (e == hipSuccess) e = seq_lds(hmm_forward_replay_wide_kernel<KT>, fb);
    if (e == hipSuccess) e = seq_lds(hmm_backward_replay_wide_kernel<KT>, fb);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hmm_prep_generic_kernel, dim3((unsigned)((T + 63) / 64)), dim3(256), 0, st, ws->lnrho, ws->npad, T, K, Kp,
                       h->rho_tm, h->mx);
    const unsigned grid = (unsigned)((n_chunks + 63) / 64);          // 16 chunks per wave, 4 waves per workgroup
    // (sweep 1: from uniform starts, nothing stored but the end vectors)
    auto replays = [&](const double* fs, const double* be, int sweep, double* f_out, double* b_out, const int* gate) {
        hipLaunchKernelGGL((hmm_forward_replay_wide_kernel<KT>), dim3(grid), dim3(256), fb, st, h->rho_tm, a_tilde, K, T, L, n_chunks,
                           fs, h->alpha_tm, h->cprime, sweep, f_out, gate);
        hipLaunchKernelGGL((hmm_backward_replay_wide_kernel<KT>), dim3(grid), dim3(256), fb, st, h->rho_tm, a_tilde, K, T, L, n_chunks,
                           be, h->alpha_tm, h->cprime, h->gamma_tm, h->w_tm, sweep, b_out, gate);
    };
    const bool two_level = n_chunks > 2 * kHmmSuper;
    auto products_path = [&](const int* gate) {
        hipLaunchKernelGGL((hmm_chunk_products_wide_kernel<KT>), dim3((unsigned)n_chunks), dim3(256), fb + 64, st, h->rho_tm, a_tilde,
                           K, T, L, n_chunks, h->prod, h->prod_t, gate);
        if (two_level) {
            // two levels: products of 64 chunk products, the sequential pass over those, every super-chunk fills in its own chunks
            const int64_t n_super = (n_chunks + kHmmSuper - 1) / kHmmSuper;
            if (hipError_t es = seq_lds(hmm_super_products_wide_kernel<KT>, fb + 64); es != hipSuccess) return es;
            hipLaunchKernelGGL((hmm_super_products_wide_kernel<KT>), dim3((unsigned)n_super), dim3(256), fb + 64, st, h->prod_t,
                               n_chunks, h->qprod, h->qprod_t, gate);
            hipLaunchKernelGGL((hmm_boundary_scan_wide_kernel<KT>), dim3(1, 2), dim3(kHmmWideScanThreads), 0, st, h->rho_tm, pi_tilde,
                               h->qprod, h->qprod_t, K, n_super, nullptr, nullptr, h->fstart_s, h->bend_s, h->cprime, h->alpha_tm,
                               h->gamma_tm, h->w_tm, gate);
            hipLaunchKernelGGL((hmm_boundary_scan_wide_kernel<KT>), dim3((unsigned)n_super, 2), dim3(kHmmWideScanThreads), 0, st,
                               h->rho_tm, pi_tilde, h->prod, h->prod_t, K, n_chunks, h->fstart_s, h->bend_s, h->fstart, h->bend,
                               h->cprime, h->alpha_tm, h->gamma_tm, h->w_tm, gate);
        } else {
            // (too few chunks for the forgetting pass: no gate to pass)
            hipLaunchKernelGGL((hmm_boundary_scan_wide_kernel<KT>), dim3(1, 2), dim3(kHmmWideScanThreads), 0, st, h->rho_tm, pi_tilde,
                               h->prod, h->prod_t, K, n_chunks, nullptr, nullptr, h->fstart, h->bend, h->cprime, h->alpha_tm,
                               h->gamma_tm, h->w_tm);
        }
        replays(h->fstart, h->bend, 0, nullptr, nullptr, gate);
        return hipSuccess;
    };
    e = forgetting_pass(
        h, st, may_try_forgetting(h, two_level), pi_tilde, n_chunks, L, L, /*staged=*/false,
        [&](int64_t, const int*) { replays(h->fstart, h->bend, 1, h->fstart, h->bend, nullptr); },
        [&](const int*) { replays(h->fstart, h->bend, 0, h->fstart2, h->bend2, nullptr); }, products_path);
    if (e != hipSuccess) return e;
    const int64_t steps = round_up((T - 1 + h->xi_waves - 1) / h->xi_waves, 4);
    const int64_t n_slabs = (T - 1 + steps - 1) / steps;
    hipLaunchKernelGGL((hmm_xi_sum_wide_kernel<KT>), dim3((unsigned)n_slabs), dim3(256), 0, st, h->alpha_tm, h->w_tm, T, steps,
                       h->xi_slabs);
    return finish_pass(h, st, T, a_tilde, n_slabs, /*w_valid=*/true, out);
}

// ---- more than 128 states, and 65 .. 128 on short sequences: one workgroup walks the sequence (hmm_generic.h) -------------
hipError_t run_generic(gmmvb_workspace* ws, gmmvb_hmm_state* h, int64_t T, const double* pi_tilde, const double* a_tilde,
                       double* out, hipStream_t st) {
    const int K = h->K, Kp = h->Kp;
    const HmmSeqShape sh = hmm_seq_shape(K);
    hipError_t e = seq_lds(hmm_seq_forward_kernel, sh.lds_bytes);
    if (e == hipSuccess) e = seq_lds(hmm_seq_backward_kernel, sh.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hmm_prep_generic_kernel, dim3((unsigned)((T + 63) / 64)), dim3(256), 0, st, ws->lnrho, ws->npad, T, K, Kp,
                       h->rho_tm, h->mx);
    hipLaunchKernelGGL(hmm_transpose_kernel, dim3((unsigned)((K * K + 255) / 256)), dim3(256), 0, st, a_tilde, K, h->a_t);
    // The forgetting pass runs the same two kernels in their chunk form, a workgroup per kHmmGenericChunk steps (L > 0; sweep 1:
    // from the uniform vector, only the end vectors stored), and the walk of the whole sequence by ONE workgroup (L = 0) only
    // behind the gate.  Sequences of at least 64 chunks.
    const int64_t L = kHmmGenericChunk;
    const int64_t n_chunks = T > 1 ? (T - 1 + L - 1) / L : 0;
    auto walks = [&](unsigned grid, int64_t l, double* fs, double* be, int sweep, double* f_out, double* b_out, const int* gate) {
        hipLaunchKernelGGL(hmm_seq_forward_kernel, dim3(grid), dim3(kHmmSeqThreads), sh.lds_bytes, st, h->rho_tm, pi_tilde, a_tilde, K,
                           Kp, T, sh.P, sh.J, sh.mat_in_lds, h->alpha_tm, h->cprime, h->gamma_tm, h->w_tm, l, fs, sweep, f_out, gate);
        hipLaunchKernelGGL(hmm_seq_backward_kernel, dim3(grid), dim3(kHmmSeqThreads), sh.lds_bytes, st, h->rho_tm, h->a_t, K, Kp, T,
                           sh.P, sh.J, sh.mat_in_lds, h->alpha_tm, h->cprime, h->gamma_tm, h->w_tm, l, be, sweep, b_out, gate);
    };
    const unsigned g = (unsigned)n_chunks;
    e = forgetting_pass(
        h, st, may_try_forgetting(h, n_chunks >= 64 && n_chunks <= h->vec_chunks), /*pi_tilde=*/nullptr, n_chunks, L, L,
        /*staged=*/false, [&](int64_t, const int*) { walks(g, L, h->fstart, h->bend, 1, h->fstart, h->bend, nullptr); },
        [&](const int*) { walks(g, L, h->fstart, h->bend, 0, h->fstart2, h->bend2, nullptr); },
        [&](const int* gate) {
            walks(1, 0, nullptr, nullptr, 0, nullptr, nullptr, gate);
            return hipSuccess;
        });
    if (e != hipSuccess) return e;
    int64_t n_slabs = 0;
    if (T > 1) {
        const int64_t steps = (T - 1 + h->xi_waves - 1) / h->xi_waves;
        n_slabs = (T - 1 + steps - 1) / steps;
        hipLaunchKernelGGL(hmm_xi_generic_kernel, dim3((unsigned)n_slabs, (unsigned)((Kp / 16) * (Kp / 16))), dim3(256), 0, st,
                           h->alpha_tm, h->w_tm, Kp, T, steps, h->xi_slabs);
    }
    return finish_pass(h, st, T, a_tilde, n_slabs, /*w_valid=*/true, out);
}

// ---- Viterbi: what the chunked paths share ----------------------------------------------------------------------------------
struct VitArgs {      // hmmvb_viterbi's arguments
    gmmvb_workspace* ws; gmmvb_hmm_state* h; int64_t n_rows;
    const double* ln_pi_tilde; const double* ln_a_tilde; int32_t* z; hipStream_t st;
};
// the status of a path whose launches have all been enqueued
int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GMMVB_OK : fail(GMMVB_EHIP, what, e);
}

// The coalescence pass (the max-plus twin of the forward-backward pass's forgetting): the best paths from all start states
// of a chunk of 256 steps normally merge inside it, and then omega behind the chunk - minus its maximum - does not depend on
// the chunk's start vector.  A sweep of the path's replay kernel from zero start vectors (no back-pointers stored) gives
// every chunk a start vector in fstart, the replay runs from those and its own end vectors (fstart2) are compared with the
// sweep's: equal to 2e-10 nats (kVitCoalesceTol), the back-pointers stand (only differences of omega enter them); otherwise
// the gate (gate_dev[1]) opens and the path's exact form runs behind it, replay included.
// replay(sweep, ends, gate) is the path's launch; omega0_threads: block of hmm_vit_omega0_kernel (0: the sweep sets the
// sequence's own start itself).
template <typename Replay>
hipError_t coalescence_pass(const VitArgs& v, int64_t chunks, unsigned omega0_threads, Replay replay) {
    gmmvb_hmm_state* h = v.h;
    int* const gate = h->gate_dev + 1;
    if (hipError_t e = hipMemsetAsync(gate, 0, sizeof(int), v.st); e != hipSuccess) return e;
    if (omega0_threads > 0)
        hipLaunchKernelGGL(hmm_vit_omega0_kernel, dim3(1), dim3(omega0_threads), 0, v.st, v.ws->lnrho, v.ws->npad, v.ln_pi_tilde, h->K,
                           h->Kp, h->fstart);
    restart_test<false>(v.st, [&] { replay(1, h->fstart, nullptr); }, [&] { replay(0, h->fstart2, nullptr); }, h->fstart, h->fstart2,
                        h->fstart, h->fstart, (chunks - 1) * h->Kp, h->Kp, kVitCoalesceTol, gate, nullptr);
    return hipSuccess;
}

// The chunked paths up to 128 states borrow the forward-backward pass's buffers, which nothing reads once that pass has
// returned: prod [chunks][Kp][Kp] chunk matrices, fstart [chunks][Kp] chunk starts, bend [chunks][Kp] bytes (trace-back maps),
// fstart_s [chunks] ints (chunk end states), and xi_slabs, qprod, bend_s (up to 64 states).
bool vit_scratch_fits(const gmmvb_hmm_state* h, int64_t chunks) {
    return chunks <= h->max_chunks &&
           chunks * (int64_t)sizeof(int) <= (h->max_chunks / kHmmSuper + 2) * h->Kp * (int64_t)sizeof(double);
}

// The path from byte back-pointers, chunk-parallel: every chunk's map from its end state to its start state, one pass over
// the maps from the last state, every chunk fills in its own steps.
void trace_back_bytes(const VitArgs& v, int64_t L, int64_t chunks, unsigned backmap_threads) {
    gmmvb_hmm_state* h = v.h;
    unsigned char* map = reinterpret_cast<unsigned char*>(h->bend);
    int* endst = reinterpret_cast<int*>(h->fstart_s);
    hipLaunchKernelGGL(hmm_vit_backmap_kernel, dim3((unsigned)chunks), dim3(backmap_threads), 0, v.st, h->phi, h->Kp, v.n_rows, L, map);
    hipLaunchKernelGGL(hmm_vit_backscan_kernel, dim3(1), dim3(256), 0, v.st, map, h->Kp, chunks, h->last_state, endst);
    hipLaunchKernelGGL(hmm_vit_fill_kernel, dim3((unsigned)((chunks + 63) / 64)), dim3(64), 0, v.st, h->phi, h->Kp, v.n_rows, L,
                       chunks, endst, v.z);
}

// ---- Viterbi, 65 .. 128 states: the chunked max-plus pass with two end states per lane and ln a~ in LDS (hmm_wide.h) --------
template <int KT>
int viterbi_wide_kt(const VitArgs& v) {
    gmmvb_workspace* ws = v.ws;
    gmmvb_hmm_state* h = v.h;
    const int64_t L = kHmmWideChunk;
    const int64_t chunks = (v.n_rows - 1 + L - 1) / L;
    double* M = h->prod;
    double* wstart = h->fstart;
    if (!vit_scratch_fits(h, chunks)) return fail(GMMVB_ESTATE, "Viterbi scratch too small for this sequence");
    const size_t lds = (size_t)h->Kp * h->Kp * sizeof(double);
    const bool coalesce = chunks >= 64 && h->spec_on && h->gate_dev != nullptr && h->fstart2 != nullptr;
    h->vit_coalesced = coalesce;
    const unsigned rgrid = (unsigned)((chunks + kVitWideWaves - 1) / kVitWideWaves);
    hipError_t ew = seq_lds(hmm_vit_chunk_wide_kernel<KT>, lds);
    if (ew == hipSuccess) ew = seq_lds(hmm_vit_replay_wide_kernel<KT>, lds);
    auto replay = [&](int sweep, double* ends, const int* gate) {
        hipLaunchKernelGGL((hmm_vit_replay_wide_kernel<KT>), dim3(rgrid), dim3(64 * kVitWideWaves), lds, v.st, ws->lnrho, ws->npad,
                           v.ln_a_tilde, wstart, h->K, v.n_rows, L, chunks, h->phi, h->last_state, sweep, ends, gate);
    };
    const int* vgate = nullptr;
    if (ew == hipSuccess && coalesce) {
        vgate = h->gate_dev + 1;
        ew = coalescence_pass(v, chunks, 128, replay);
    }
    if (ew != hipSuccess) return fail(GMMVB_EHIP, "chunked viterbi (65 .. 128 states: LDS size)", ew);
    hipLaunchKernelGGL((hmm_vit_chunk_wide_kernel<KT>),
                       dim3((unsigned)chunks, (unsigned)((h->K + 4 * kVitWideWaves - 1) / (4 * kVitWideWaves))),
                       dim3(64 * kVitWideWaves), lds, v.st, ws->lnrho, ws->npad, v.ln_a_tilde, h->K, v.n_rows, L, M, vgate);
    hipLaunchKernelGGL((hmm_vit_scan_wide_kernel<KT>), dim3(1), dim3(kHmmWideScanThreads), 0, v.st, ws->lnrho, ws->npad, v.ln_pi_tilde,
                       M, h->K, chunks, wstart, vgate);
    replay(0, nullptr, vgate);
    trace_back_bytes(v, L, chunks, 128);
    return launched("chunked viterbi launch (65 .. 128 states)");
}
int viterbi_wide(const VitArgs& v) { return dispatch_kt<5, 8>(v.h->KT, [&](auto kt) { return viterbi_wide_kt<decltype(kt)::value>(v); }); }

// ---- Viterbi, more than 128 states (and 65 .. 128 on short sequences): hmm_generic.h, 16-bit back-pointers ---------------
int viterbi_generic(const VitArgs& v) {
    gmmvb_workspace* ws = v.ws;
    gmmvb_hmm_state* h = v.h;
    const HmmSeqShape sh = hmm_seq_shape(h->K);
    hipError_t eg = seq_lds(hmm_seq_viterbi_kernel, sh.lds_bytes);
    if (eg != hipSuccess) return fail(GMMVB_EHIP, "viterbi (LDS size)", eg);
    // chunk form (l > 0, a workgroup per chunk) through the coalescence pass, the walk of the whole sequence by one workgroup
    // (l = 0) behind its gate; the path is traced back chunk-parallel either way
    const int64_t L = kHmmGenericChunk;
    const int64_t chunks = v.n_rows > 1 ? (v.n_rows - 1 + L - 1) / L : 0;
    const bool chunked = chunks >= 2 && chunks <= h->vec_chunks && h->fstart2 != nullptr;
    const bool coalesce = chunked && chunks >= 64 && h->spec_on && h->gate_dev != nullptr;
    h->vit_coalesced = coalesce;
    auto walk = [&](unsigned grid, int64_t l, double* starts, int sweep, double* ends, const int* gate) {
        hipLaunchKernelGGL(hmm_seq_viterbi_kernel, dim3(grid), dim3(kHmmSeqThreads), sh.lds_bytes, v.st, ws->lnrho, ws->npad,
                           v.ln_pi_tilde, v.ln_a_tilde, h->K, v.n_rows, sh.P, sh.J, sh.mat_in_lds, h->phi16, h->last_state, l, h->Kp,
                           starts, sweep, ends, gate);
    };
    const int* vgate = nullptr;
    if (coalesce) {
        vgate = h->gate_dev + 1;
        if (coalescence_pass(v, chunks, 0, [&](int sweep, double* ends, const int* gate) {
                walk((unsigned)chunks, L, h->fstart, sweep, ends, gate);
            }) != hipSuccess)
            return fail(GMMVB_EHIP, "viterbi (gate reset)");
    }
    walk(1, 0, nullptr, 0, nullptr, vgate);
    if (chunked) {
        // scratch: the forward-backward pass's w array ([npad][Kp] doubles; nothing reads it once gmmvb_estep has run again)
        unsigned short* map = reinterpret_cast<unsigned short*>(h->w_tm);        // [chunks][K]
        int* endst = reinterpret_cast<int*>(h->w_tm + (chunks * (int64_t)h->K + 3) / 4 + 1);      // [chunks]
        hipLaunchKernelGGL(hmm_seq_backmap_kernel, dim3((unsigned)chunks), dim3(256), 0, v.st, h->phi16, h->K, v.n_rows, L, map);
        hipLaunchKernelGGL(hmm_seq_backscan_kernel, dim3(1), dim3(64), 0, v.st, map, h->K, chunks, h->last_state, endst);
        hipLaunchKernelGGL(hmm_seq_fill_kernel, dim3((unsigned)((chunks + 63) / 64)), dim3(64), 0, v.st, h->phi16, h->K, v.n_rows, L,
                           chunks, endst, v.z);
    } else {
        hipLaunchKernelGGL(hmm_seq_backtrack_kernel, dim3(1), dim3(64), 0, v.st, h->phi16, h->K, v.n_rows, h->last_state, v.z);
    }
    return launched("viterbi launch (generic)");
}

// ---- Viterbi, up to 64 states (hmm.h, hmm_vit_*) ------------------------------------------------------------------------------
constexpr int64_t kVitChunkedFrom = 512;       // shorter sequences: the single sequential wave
constexpr int64_t kVitLongFrom = 65536;        // from here chunks of 256 steps (and the coalescence pass), below of 32

// the chunked max-plus scan
template <int KT>
int viterbi_chunked_kt(const VitArgs& v) {
    gmmvb_workspace* ws = v.ws;
    gmmvb_hmm_state* h = v.h;
    const int64_t L = v.n_rows >= kVitLongFrom ? 256 : 32;
    const int64_t chunks = (v.n_rows - 1 + L - 1) / L;
    double* M = h->prod;
    double* wstart = h->fstart;
    if (!vit_scratch_fits(h, chunks)) return fail(GMMVB_ESTATE, "Viterbi scratch too small for this sequence");
    // chunk matrices: up to 32 states with a lane per start state (hmm_vit_chunk_lane_kernel), beyond with a wave per
    // (chunk, start state).  Chunk starts: with more than two super-chunks through super-chunk products (a sequential
    // pass over chunks / 64 products instead of over every chunk), else the single workgroup's pass.
    const int64_t supers = (chunks + kHmmSuper - 1) / kHmmSuper;
    const bool two_level = supers > 2 && h->qprod != nullptr && h->bend_s != nullptr;
    double* a_pad = h->xi_slabs;                                     // [Kp][Kp]
    double* sstart = h->bend_s;                                      // [supers][Kp]
    const bool coalesce = L == 256 && chunks >= 64 && h->spec_on && h->gate_dev != nullptr && h->fstart2 != nullptr;
    h->vit_coalesced = coalesce;
    auto replay = [&](int sweep, double* ends, const int* gate) {
        hipLaunchKernelGGL((hmm_vit_replay_kernel<KT>), dim3((unsigned)chunks), dim3(64), 0, v.st, ws->lnrho, ws->npad, v.ln_a_tilde,
                           wstart, h->K, v.n_rows, L, chunks, h->phi, h->last_state, sweep, ends, gate);
    };
    const int* vgate = nullptr;
    if (coalesce) {
        vgate = h->gate_dev + 1;
        if (coalescence_pass(v, chunks, 64, replay) != hipSuccess) return fail(GMMVB_EHIP, "viterbi (gate reset)");
    }
    if (KT <= 2) {
        constexpr int KPL = KT <= 1 ? 16 : 32;
        hipLaunchKernelGGL(hmm_vit_pad_kernel, dim3((KPL * KPL + 255) / 256), dim3(256), 0, v.st, v.ln_a_tilde, h->K, KPL, a_pad);
        hipLaunchKernelGGL((hmm_vit_chunk_lane_kernel<KPL>), dim3((unsigned)((chunks + 64 / KPL - 1) / (64 / KPL))), dim3(64), 0, v.st,
                           ws->lnrho, ws->npad, a_pad, h->K, v.n_rows, L, chunks, M, vgate);
    } else {
        hipLaunchKernelGGL((hmm_vit_chunk_kernel<KT>), dim3((unsigned)chunks, (unsigned)((h->K + 3) / 4)), dim3(256), 0, v.st,
                           ws->lnrho, ws->npad, v.ln_a_tilde, h->K, v.n_rows, L, M, vgate);
    }
    if (two_level) {
        hipLaunchKernelGGL((hmm_vit_super_kernel<16 * KT>), dim3((unsigned)supers), dim3(256), 0, v.st, M, h->K, chunks, h->qprod,
                           vgate);
        hipLaunchKernelGGL((hmm_vit_scan2_kernel<16 * KT>), dim3(1), dim3(64), 0, v.st, ws->lnrho, ws->npad, v.ln_pi_tilde, h->qprod,
                           h->K, supers, sstart, vgate);
        hipLaunchKernelGGL((hmm_vit_fill2_kernel<16 * KT>), dim3((unsigned)supers), dim3(64), 0, v.st, M, h->K, chunks, sstart, wstart,
                           vgate);
    } else {
        hipLaunchKernelGGL((hmm_vit_scan_kernel<KT>), dim3(1), dim3(256), 0, v.st, ws->lnrho, ws->npad, v.ln_pi_tilde, M, h->K, chunks,
                           wstart, vgate);
    }
    replay(0, nullptr, vgate);
    trace_back_bytes(v, L, chunks, 64);
    return launched("chunked viterbi launch");
}
int viterbi_chunked(const VitArgs& v) { return dispatch_kt<1, 4>(v.h->KT, [&](auto kt) { return viterbi_chunked_kt<decltype(kt)::value>(v); }); }

// the single sequential wave
template <int KT>
int viterbi_wave_kt(const VitArgs& v) {
    gmmvb_hmm_state* h = v.h;
    hipLaunchKernelGGL((hmm_viterbi_forward_kernel<KT>), dim3(1), dim3(64), 0, v.st, v.ws->lnrho, v.ws->npad, v.ln_pi_tilde,
                       v.ln_a_tilde, h->K, v.n_rows, h->phi, h->last_state);
    hipLaunchKernelGGL(hmm_viterbi_backtrack_kernel, dim3(1), dim3(256), 0, v.st, h->phi, h->Kp, v.n_rows, h->last_state, v.z);
    return launched("viterbi launch");
}
int viterbi_wave(const VitArgs& v) { return dispatch_kt<1, 4>(v.h->KT, [&](auto kt) { return viterbi_wave_kt<decltype(kt)::value>(v); }); }

}  // namespace

extern "C" {

int64_t hmmvb_out_len(int K) { return K < 1 ? -1 : (int64_t)K * K + 2 * (int64_t)K + 1; }

int hmmvb_enable(gmmvb_workspace* ws) {
    if (!ws) return fail(GMMVB_EINVAL, "null argument");
    if (ws->hmm) return GMMVB_OK;
    if (ws->scratch && ws->scratch->refs > 1)
        return fail(GMMVB_EUNSUPPORTED, "HMM: the time axis does not tile (this workspace belongs to a tile group)");
    if (ws->K > 65535) return fail(GMMVB_EUNSUPPORTED, "HMM: at most 65535 states (16-bit back-pointers)");
    gmmvb_hmm_state* h = new (std::nothrow) gmmvb_hmm_state();
    if (!h) return fail(GMMVB_ENOMEM, "host allocation failed");
    h->K = ws->K;
    h->KT = (ws->K + 15) / 16;
    h->Kp = 16 * h->KT;
    h->npad = ws->npad;
    h->generic = ws->K > 64;                    // (the chunk-parallel kernels hold K x K products in registers)
    h->wide = ws->K > 64 && ws->K <= 128 && dev_env("GMMVB_HMM_WIDE_OFF") == nullptr;      // hmm_wide.h (developer switch: off)
    // (65 .. 128 states: chunks of 256 steps, or of 128 while those do not fill the CUs - run_wide)
    h->max_chunks = h->wide ? std::min<int64_t>(std::max<int64_t>(64 * (int64_t)ws->num_cu, ws->npad / kHmmWideChunk), ws->npad / 128) + 2
                            : (h->generic ? 1 : ws->npad / 16 + 2);          // narrow_chunk_len >= 16
    h->xi_waves = h->generic ? std::max<int64_t>(16, std::min<int64_t>(4 * (int64_t)ws->num_cu, (int64_t(1) << 27) / ((int64_t)h->Kp * h->Kp)))
                             : 16 * (int64_t)ws->num_cu;       // four xi-sum waves per SIMD: the kernel streams two [T][Kp] arrays and a wave
                                                               // has one load group in flight (round 4; one wave per SIMD: 1.9 ms, 2.6 TB/s)
    // room for one xi slab per replay wave (hmm.h H5 XI): sequences past 2^15 steps have chunks of kHmmLongChunk steps, 16 to a
    // wave; shorter ones at most ~850 chunks (narrow_chunk_len)
    h->xi_slab_cap = std::max<int64_t>(h->xi_waves + 4, h->generic ? 0 : h->npad / (16 * (kHmmLongChunk / 2)) + 72);
    h->xi_separate = dev_env("GMMVB_HMM_XI_SEPARATE") != nullptr;
    // chunk boundary vectors: more than 128 states walk chunks of kHmmGenericChunk steps in the forgetting pass (run_generic)
    h->vec_chunks = (h->generic && !h->wide) ? h->npad / kHmmGenericChunk + 2 : h->max_chunks;
    for (const HmmBuf& b : hmm_buffers(h)) {
        if (b.n == 0) continue;
        hipError_t e = hipMalloc((void**)b.p, (size_t)b.n * sizeof(double));
        if (e != hipSuccess) {
            hmm_state_destroy(h);
            return fail(GMMVB_ENOMEM, "hipMalloc (HMM buffers)", e);
        }
        h->bytes += b.n * (int64_t)sizeof(double);
    }
    hipError_t e2 = h->generic ? hipMalloc((void**)&h->phi16, (size_t)(h->npad * ws->K) * sizeof(unsigned short))
                               : hipMalloc((void**)&h->phi, (size_t)(h->npad * h->Kp));
    if (e2 == hipSuccess && h->wide) {          // (65 .. 128 states: byte back-pointers of the chunked Viterbi pass)
        e2 = hipMalloc((void**)&h->phi, (size_t)(h->npad * h->Kp));
        h->bytes += h->npad * h->Kp;
    }
    if (e2 == hipSuccess) e2 = hipMalloc((void**)&h->last_state, sizeof(int));
    if (e2 == hipSuccess && h->generic && !h->wide) {        // (their padding entries are never written and are compared)
        for (double* p : {h->fstart, h->bend, h->fstart2, h->bend2})
            if (e2 == hipSuccess) e2 = hipMemset(p, 0, (size_t)(h->vec_chunks * h->Kp) * sizeof(double));
    }
    if (e2 == hipSuccess) {      // the forgetting pass's gate (forgetting_pass): device flag, pinned copy, event
        h->spec_on = dev_env("GMMVB_HMM_FORGETTING_OFF") == nullptr;
        if (const char* v = dev_env("GMMVB_HMM_SWEEP_LEN")) h->sweep_len = std::max<int64_t>(1, std::atoll(v));      // developer switch
        e2 = hipMalloc((void**)&h->gate_dev, 4 * sizeof(int));      // [0] forward-backward (exact form), [1] Viterbi, [2] forward-backward (whole-chunk stage)
        if (e2 == hipSuccess) e2 = hipHostMalloc((void**)&h->gate_host, 2 * sizeof(int));
        if (e2 == hipSuccess) e2 = hipEventCreateWithFlags(&h->gate_ev, hipEventDisableTiming);
        if (e2 == hipSuccess) h->gate_host[0] = h->gate_host[1] = 0;
    }
    if (e2 != hipSuccess) {
        hmm_state_destroy(h);
        return fail(GMMVB_ENOMEM, "hipMalloc (Viterbi buffers)", e2);
    }
    h->bytes += (h->generic ? 2 * h->npad * ws->K : h->npad * h->Kp) + 4;
    ws->hmm = h;
    ws->bytes += h->bytes;
    return GMMVB_OK;
}

int hmmvb_viterbi(gmmvb_workspace* ws, int64_t n_rows, const double* ln_pi_tilde_dev, const double* ln_a_tilde_dev,
                  int32_t* z_dev, void* stream) {
    if (!ws || !ln_pi_tilde_dev || !ln_a_tilde_dev || !z_dev) return fail(GMMVB_EINVAL, "null argument");
    if (!ws->hmm) return fail(GMMVB_ESTATE, "hmmvb_enable has not been called");
    if (ws->e_state == 4)
        return fail(GMMVB_ESTATE, "the last gmmvb_estep formed no ln rho array (hmmvb_emission_target 1): run it with target 0");
    if (ws->e_state != 1 || ws->e_rows != n_rows)
        return fail(GMMVB_ESTATE, "no emission ln rho for these rows: call gmmvb_estep first");
    gmmvb_hmm_state* h = ws->hmm;
    h->vit_coalesced = false;
    // the pass takes the forward-backward pass's buffers as scratch (chunk products, boundary vectors, xi slabs, w_tm): whatever
    // that pass left is gone - said explicitly, not only through e_state (hmmvb_readout checks gamma_rows)
    h->w_valid = false;
    h->gamma_rows = 0;
    h->gamma_cm_valid = false;
    const VitArgs v{ws, h, n_rows, ln_pi_tilde_dev, ln_a_tilde_dev, z_dev, (hipStream_t)stream};
    if (h->wide && h->phi && n_rows >= kHmmWideMinSteps) return viterbi_wide(v);
    if (h->generic) return viterbi_generic(v);
    return n_rows >= kVitChunkedFrom ? viterbi_chunked(v) : viterbi_wave(v);
}

int hmmvb_last_viterbi_pass(gmmvb_workspace* ws) {
    if (!ws || !ws->hmm) return -2;
    if (!ws->hmm->vit_coalesced) return -1;
    int g = 0;
    if (hipMemcpy(&g, ws->hmm->gate_dev + 1, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -2;      // (synchronises)
    return g;
}

int hmmvb_last_boundary_pass(gmmvb_workspace* ws) {
    if (!ws || !ws->hmm) return -2;
    gmmvb_hmm_state* h = ws->hmm;
    if (!consume_gate(h, /*wait=*/true)) return -2;
    return h->last_gate;
}

int hmmvb_skip_h(gmmvb_workspace* ws, int skip) {
    if (!ws) return fail(GMMVB_EINVAL, "null argument");
    if (!ws->hmm) return fail(GMMVB_ESTATE, "hmmvb_enable has not been called");
    ws->hmm_skip_h = skip != 0;
    return GMMVB_OK;
}

int hmmvb_emission_target(gmmvb_workspace* ws, int fused, int* in_effect) {
    if (!ws) return fail(GMMVB_EINVAL, "null argument");
    if (!ws->hmm) return fail(GMMVB_ESTATE, "hmmvb_enable has not been called");
    ws->hmm->fuse_emission = fused != 0 && ws->T == 1 && !ws->wide && dev_env("GMMVB_HMM_FUSED_EMISSION_OFF") == nullptr;
    if (in_effect) *in_effect = hmm_fused_emission(ws->hmm) ? 1 : 0;
    return GMMVB_OK;
}

int hmmvb_forward_backward(gmmvb_workspace* ws, int64_t n_rows, const double* pi_tilde_dev, const double* a_tilde_dev,
                           double* out_dev, void* stream) {
    if (!ws || !pi_tilde_dev || !a_tilde_dev || !out_dev) return fail(GMMVB_EINVAL, "null argument");
    if (!ws->hmm) return fail(GMMVB_ESTATE, "hmmvb_enable has not been called");
    if ((ws->e_state != 1 && ws->e_state != 4) || ws->e_rows != n_rows)
        return fail(GMMVB_ESTATE, "no emission ln rho for these rows: call gmmvb_estep first");
    gmmvb_hmm_state* h = ws->hmm;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    const char* what = "HMM forward-backward launch";
    consume_gate(h, /*wait=*/false);      // what the last forgetting pass's gate means for this call
    if (h->wide && n_rows >= kHmmWideMinSteps) {
        what = "HMM forward-backward launch (65 .. 128 states)";
        e = dispatch_kt<5, 8>(h->KT, [&](auto kt) {
            return run_wide<decltype(kt)::value>(ws, h, n_rows, pi_tilde_dev, a_tilde_dev, out_dev, st);
        });
    } else if (h->generic) {
        what = "HMM forward-backward launch (generic)";
        e = run_generic(ws, h, n_rows, pi_tilde_dev, a_tilde_dev, out_dev, st);
    } else {
        if (h->KT < 1 || h->KT > 4) return fail(GMMVB_EUNSUPPORTED, "K > 64");
        e = dispatch_kt<1, 4>(h->KT, [&](auto kt) {
            return run<decltype(kt)::value>(ws, h, n_rows, pi_tilde_dev, a_tilde_dev, out_dev, st);
        });
    }
    if (e != hipSuccess) return fail(GMMVB_EHIP, what, e);
    ws->e_state = 3;
    return GMMVB_OK;
}

int hmmvb_readout(gmmvb_workspace* ws, int what, int64_t row0, int64_t n_rows, const double* a_tilde_dev, double* out_dev,
                  void* stream) {
    if (!ws || !ws->hmm || !out_dev) return fail(GMMVB_EINVAL, "null argument");
    if (what != 0 && what != 1 && what != 3) return fail(GMMVB_EINVAL, "what must be 0 (alpha), 1 (beta) or 3 (xi)");
    if (what == 3 && !a_tilde_dev) return fail(GMMVB_EINVAL, "a_tilde_dev is needed for xi");
    if (ws->e_state != 3 || row0 < 0 || n_rows < 1 || row0 + n_rows > ws->e_rows || row0 + n_rows > ws->hmm->gamma_rows)
        return fail(GMMVB_ESTATE, "row range outside the last hmmvb_forward_backward (or hmmvb_viterbi has reused its buffers)");
    gmmvb_hmm_state* h = ws->hmm;
    const int64_t total = n_rows * h->K * (what == 3 ? h->K : 1);
    hipLaunchKernelGGL(hmm_readout_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->alpha_tm,
                       h->gamma_tm, h->w_valid ? h->w_tm : nullptr, a_tilde_dev, h->K, h->Kp, what, row0, n_rows, out_dev, h->rho_tm,
                       h->cprime);
    return launched("hmm_readout launch");
}

/* Read-outs of the last forward-backward pass for rows [row0, row0 + n_rows): alpha / beta~ are not kept in
 * natural order; this returns alpha (mode 0) or c' (mode 1, [n_rows]) for tests. */
int hmmvb_debug_readout(gmmvb_workspace* ws, int what, int64_t row0, int64_t n_rows, double* out_dev, void* stream) {
    if (!ws || !ws->hmm || !out_dev) return fail(GMMVB_EINVAL, "null argument");
    if (ws->e_state != 3 || row0 < 0 || n_rows < 1 || row0 + n_rows > ws->e_rows) return fail(GMMVB_EINVAL, "bad range");
    gmmvb_hmm_state* h = ws->hmm;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (what == 1) {
        e = hipMemcpyAsync(out_dev, h->cprime + row0, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToDevice, st);
    } else if (what == 2) {
        e = hipMemcpyAsync(out_dev, h->mx + row0, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToDevice, st);
    } else {
        // alpha in lane order, [n_rows][Kp]; the caller un-permutes (positions: hmm_pos)
        e = hipMemcpyAsync(out_dev, h->alpha_tm + row0 * h->Kp, (size_t)n_rows * h->Kp * sizeof(double),
                           hipMemcpyDeviceToDevice, st);
    }
    if (e != hipSuccess) return fail(GMMVB_EHIP, "debug readout", e);
    return GMMVB_OK;
}

}  // extern "C"

