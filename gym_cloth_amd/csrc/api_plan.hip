// api_plan.hip -- the cross-entropy planner over forked cloths (clothhip.h: clothhip_plan_cem, clothhip_plan_sample, clothhip_plan_refit): the
// only unit that sees the planner's kernels (cloth_plan.hpp). The loop is made of entries that exist -- clothhip_fork, an episode launch (begin_launch)
// on a device-resident table -- and the two kernels; it ends each launch through run_actions_end_on_device (both api_run.hip), so the records are
// scored where they lie and nothing comes back from the device before the last iteration is done.
#include <hip/hip_runtime.h>

#include <cmath>

#include "api_handle.hpp"
#include "cloth_plan.hpp"

// the bounds of ClothPlanParams every entry checks (clothhip.h: BOUNDS); whole: also the fields only the loop and the refit read
static int check_plan_params(const ClothPlanParams *p, bool whole) {
    if (!p) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (p->horizon < 1 || p->horizon > PLAN_MAX_H) return fail(CLOTHHIP_EINVAL, "horizon %d outside [1, %d]", p->horizon, PLAN_MAX_H);
    if (p->n_candidates < 2 || p->n_candidates > PLAN_MAX_K) return fail(CLOTHHIP_EINVAL, "n_candidates %d outside [2, %d]", p->n_candidates, PLAN_MAX_K);
    if (!whole) return 0;
    if (p->n_elite < 1 || p->n_elite > p->n_candidates) return fail(CLOTHHIP_EINVAL, "n_elite %d outside [1, n_candidates = %d]", p->n_elite, p->n_candidates);
    if (p->n_iters < 1) return fail(CLOTHHIP_EINVAL, "n_iters %d < 1", p->n_iters);
    if ((uint64_t)p->iter0 + (uint64_t)p->n_iters > ((uint64_t)1 << 31)) return fail(CLOTHHIP_EINVAL, "iter0 + n_iters exceeds 2^31");
    if (!(p->alpha > 0.0 && p->alpha <= 1.0)) return fail(CLOTHHIP_EINVAL, "alpha %g outside (0, 1]", p->alpha);
    if (!std::isfinite(p->penalty)) return fail(CLOTHHIP_EINVAL, "penalty is not finite");
    for (int a = 0; a < 4; a++)
        if (!(std::isfinite(p->min_std[a]) && p->min_std[a] >= 0.0)) return fail(CLOTHHIP_EINVAL, "min_std[%d] = %g: finite and >= 0", a, p->min_std[a]);
    return 0;
}
// mean finite, std finite and >= 0, for the envs that are planned (done NULL: all)
static int check_distribution(const double *mean, const double *sdev, const uint8_t *done, int64_t E, int H) {
    for (int64_t e = 0; e < E; e++) {
        if (done && done[e]) continue;
        for (int64_t i = e * H * 4; i < (e + 1) * H * 4; i++) {
            if (!std::isfinite(mean[i])) return fail(CLOTHHIP_EINVAL, "mean of env %lld is not finite", (long long)e);
            if (!(std::isfinite(sdev[i]) && sdev[i] >= 0.0)) return fail(CLOTHHIP_EINVAL, "std of env %lld is not finite and >= 0", (long long)e);
        }
    }
    return 0;
}
static int check_act_bounds(const double *lo, const double *hi) {
    for (int a = 0; a < 4; a++)
        if (!(std::isfinite(lo[a]) && std::isfinite(hi[a]) && lo[a] <= hi[a])) return fail(CLOTHHIP_EINVAL, "act_low / act_high [%d]: finite, low <= high", a);
    return 0;
}

static int launch_sample(clothhip_handle *h, const ClothPlanParams *p, const double *lo, const double *hi, int E, uint32_t iter, double *d_x) {
    PlanSampleArgs a;
    a.mean = h->plan.d_mean; a.std = h->plan.d_std; a.x = d_x;
    for (int k = 0; k < 4; k++) { a.lo[k] = lo[k]; a.hi[k] = hi[k]; }
    a.seed = p->seed; a.iter = iter; a.E = E; a.K = p->n_candidates; a.H = p->horizon;
    const int64_t n = (int64_t)E * a.K * a.H * 4;
    hipLaunchKernelGGL(k_plan_sample, dim3((unsigned)((n + PLAN_THREADS - 1) / PLAN_THREADS)), dim3(PLAN_THREADS), 0, h->stream, a);
    HIPCHECK(hipGetLastError());
    return 0;
}

static int launch_refit(clothhip_handle *h, const ClothPlanParams *p, int E, const double *d_x, const ClothStepRecord *d_rec, double *d_scores,
                        bool have_done, bool with_best, bool with_elite, bool first) {
    PlanRefitArgs a;
    a.x = d_x; a.rec = d_rec; a.scores = d_scores; a.done = have_done ? (const uint8_t *)h->plan.d_done : nullptr;
    a.mean = h->plan.d_mean; a.std = h->plan.d_std;
    a.best_actions = with_best ? (double *)h->plan.d_best_a : nullptr; a.best_score = with_best ? (double *)h->plan.d_best_s : nullptr;
    a.elite = with_elite ? (uint8_t *)h->plan.d_elite : nullptr; a.top = with_elite ? (int32_t *)h->plan.d_top : nullptr;
    a.alpha = p->alpha; a.beta = 1.0 - p->alpha; a.penalty = p->penalty;
    for (int k = 0; k < 4; k++) a.min_std[k] = p->min_std[k];
    a.E = E; a.K = p->n_candidates; a.H = p->horizon; a.M = p->n_elite; a.first = first ? 1 : 0;
    hipLaunchKernelGGL(k_plan_refit, dim3(E), dim3(PLAN_THREADS), 0, h->stream, a);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int clothhip_plan_sample(clothhip_handle *h, const ClothPlanParams *params, const double act_low[4], const double act_high[4], int32_t E,
                                    int32_t it, const double *mean, const double *sdev, double *x_out) {
    if (!h || !act_low || !act_high || !mean || !sdev || !x_out) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_plan_params(params, false)) return rc;
    if (E < 1) return fail(CLOTHHIP_EINVAL, "E = %d < 1", E);
    if (it < 0 || (uint64_t)params->iter0 + (uint64_t)it >= ((uint64_t)1 << 31)) return fail(CLOTHHIP_EINVAL, "iteration %d: iter0 + it must lie in [0, 2^31)", it);
    if (int rc = check_act_bounds(act_low, act_high)) return rc;
    if (int rc = check_distribution(mean, sdev, nullptr, E, params->horizon)) return rc;
    if (int rc = check_idle(h)) return rc;
    const size_t nd = (size_t)E * params->horizon * 4 * 8, nx = nd * params->n_candidates;
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (int rc = h->plan.d_mean.reserve(nd)) return rc;
    if (int rc = h->plan.d_std.reserve(nd)) return rc;
    if (int rc = h->plan.d_x.reserve(nx)) return rc;
    HIPCHECK(hipMemcpyAsync(h->plan.d_mean, mean, nd, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->plan.d_std, sdev, nd, hipMemcpyHostToDevice, h->stream));
    if (int rc = launch_sample(h, params, act_low, act_high, E, params->iter0 + (uint32_t)it, h->plan.d_x)) return rc;
    HIPCHECK(hipMemcpyAsync(x_out, h->plan.d_x, nx, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_plan_refit(clothhip_handle *h, const ClothPlanParams *params, int32_t E, const double *x, const double *scores,
                                   const uint8_t *done, double *mean, double *sdev, uint8_t *elite, int32_t *top) {
    if (!h || !x || !scores || !mean || !sdev) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_plan_params(params, true)) return rc;
    if (E < 1) return fail(CLOTHHIP_EINVAL, "E = %d < 1", E);
    const int K = params->n_candidates, H = params->horizon;
    if (int rc = check_distribution(mean, sdev, done, E, H)) return rc;
    for (int64_t i = 0; i < (int64_t)E * K; i++)
        if (std::isnan(scores[i])) return fail(CLOTHHIP_EINVAL, "scores[%lld][%lld] is NaN", (long long)(i / K), (long long)(i % K));
    for (int64_t i = 0; i < (int64_t)E * K * H * 4; i++)
        if (!std::isfinite(x[i])) return fail(CLOTHHIP_EINVAL, "the action table holds a value that is not finite (element %lld)", (long long)i);
    if (int rc = check_idle(h)) return rc;
    const size_t nd = (size_t)E * H * 4 * 8, nx = nd * K, ns = (size_t)E * K * 8;
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (int rc = h->plan.d_mean.reserve(nd)) return rc;
    if (int rc = h->plan.d_std.reserve(nd)) return rc;
    if (int rc = h->plan.d_x.reserve(nx)) return rc;
    if (int rc = h->plan.d_scores.reserve(ns)) return rc;
    if (int rc = h->plan.d_done.reserve((size_t)E)) return rc;
    if (int rc = h->plan.d_elite.reserve((size_t)E * K)) return rc;
    if (int rc = h->plan.d_top.reserve((size_t)E * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->plan.d_mean, mean, nd, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->plan.d_std, sdev, nd, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->plan.d_x, x, nx, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->plan.d_scores, scores, ns, hipMemcpyHostToDevice, h->stream));
    if (done) HIPCHECK(hipMemcpyAsync(h->plan.d_done, done, (size_t)E, hipMemcpyHostToDevice, h->stream));
    if (int rc = launch_refit(h, params, E, h->plan.d_x, nullptr, h->plan.d_scores, done != nullptr, false, true, true)) return rc;
    HIPCHECK(hipMemcpyAsync(mean, h->plan.d_mean, nd, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(sdev, h->plan.d_std, nd, hipMemcpyDeviceToHost, h->stream));
    if (elite) HIPCHECK(hipMemcpyAsync(elite, h->plan.d_elite, (size_t)E * K, hipMemcpyDeviceToHost, h->stream));
    if (top) HIPCHECK(hipMemcpyAsync(top, h->plan.d_top, (size_t)E * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_plan_cem(clothhip_handle *scratch, clothhip_handle *src, const ClothEpisodeParams *ep, const ClothPlanParams *params,
                                 const int32_t *num_steps, const uint8_t *done, double *mean, double *sdev, double *best_actions, double *best_score,
                                 double *scores_out, double *cands_out) {
    if (!scratch || !src || !ep || !num_steps || !done || !mean || !sdev || !best_actions || !best_score) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_plan_params(params, true)) return rc;
    if (scratch == src) return fail(CLOTHHIP_EINVAL, "the scratch handle must not be the source handle");
    const int E = src->E, K = params->n_candidates, H = params->horizon, n_iters = params->n_iters;
    const int64_t EK = (int64_t)E * K;
    if ((int64_t)scratch->E != EK) return fail(CLOTHHIP_EINVAL, "the scratch handle has %d cloths, %d envs x %d candidates need %lld", scratch->E, E, K, (long long)EK);
    if (scratch->device != src->device) return fail(CLOTHHIP_EINVAL, "the scratch handle is on device %d, the source on %d", scratch->device, src->device);
    if (scratch->precision != src->precision) return fail(CLOTHHIP_EINVAL, "the scratch handle has another precision than the source");
    if (scratch->N != src->N) return fail(CLOTHHIP_EINVAL, "the scratch handle's grid has %d points a side, the source's %d", scratch->N, src->N);
    {
        ClothParams a = scratch->prm, b = src->prm;
        a._pad = b._pad = 0;
        if (memcmp(&a, &b, sizeof(a)) != 0) return fail(CLOTHHIP_EINVAL, "the scratch handle was created with other ClothParams than the source");
    }
    if (!(ep->reduce_factor > 0) || ep->max_actions < 1) return fail(CLOTHHIP_EINVAL, "bad episode parameters");
    if (int rc = check_act_bounds(ep->act_low, ep->act_high)) return rc;
    if (int rc = check_distribution(mean, sdev, done, E, H)) return rc;
    if (src->epi.last.pending || scratch->epi.last.pending) return fail(CLOTHHIP_ESTATE, "a clothhip_run_actions_begin is in flight on the %s handle: call clothhip_run_actions_end first", src->epi.last.pending ? "source" : "scratch");
    if (scratch->relaxed) return fail(CLOTHHIP_ESTATE, "clothhip_set_relaxed_order: the relaxed-order companion is a bench-only kernel, not a model to plan with");
    if (!fused_supported(*scratch)) return fail(CLOTHHIP_ESTATE, "n_side %d: the scratch handle's stepper variant cannot run episode launches (clothhip_fused_supported)", scratch->N);
    {
        std::vector<uint8_t> parked((size_t)E);
        if (int rc = clothhip_in_flight(src, parked.data())) return rc;
        for (int e = 0; e < E; e++)
            if (parked[e] && !done[e]) return fail(CLOTHHIP_ESTATE, "env %d holds an operation a time slice cut (clothhip_in_flight): plan between whole actions", e);
    }
    // from here on only the scratch handle changes
    const size_t nd = (size_t)E * H * 4 * 8, nx = nd * K, ns = (size_t)EK * 8;
    HIPCHECK(hipSetDevice(scratch->device));
    HIPCHECK(hipStreamSynchronize(scratch->stream));
    clothhip_handle::Plan &P = scratch->plan;
    if (int rc = P.d_mean.reserve(nd)) return rc;
    if (int rc = P.d_std.reserve(nd)) return rc;
    if (int rc = P.d_best_a.reserve(nd)) return rc;
    if (int rc = P.d_best_s.reserve((size_t)E * 8)) return rc;
    if (int rc = P.d_done.reserve((size_t)E)) return rc;
    if (int rc = P.d_x.reserve(cands_out ? nx * n_iters : nx)) return rc;
    if (int rc = P.d_scores.reserve(ns * n_iters)) return rc;
    HIPCHECK(hipMemcpyAsync(P.d_mean, mean, nd, hipMemcpyHostToDevice, scratch->stream));
    HIPCHECK(hipMemcpyAsync(P.d_std, sdev, nd, hipMemcpyHostToDevice, scratch->stream));
    HIPCHECK(hipMemcpyAsync(P.d_done, done, (size_t)E, hipMemcpyHostToDevice, scratch->stream));
    HIPCHECK(hipStreamSynchronize(scratch->stream));
    std::vector<int32_t> idx((size_t)2 * EK), steps_rep((size_t)EK);
    std::vector<uint8_t> done_rep((size_t)EK);
    for (int64_t s = 0; s < EK; s++) {
        idx[s] = (int32_t)s; idx[EK + s] = (int32_t)(s / K);
        steps_rep[s] = num_steps[s / K]; done_rep[s] = done[s / K];
    }
    for (int it = 0; it < n_iters; it++) {
        double *d_x = (double *)P.d_x + (cands_out ? (size_t)it * (nx / 8) : 0);
        double *d_s = (double *)P.d_scores + (size_t)it * EK;
        if (int rc = launch_sample(scratch, params, ep->act_low, ep->act_high, E, params->iter0 + (uint32_t)it, d_x)) return rc;
        if (int rc = clothhip_fork(scratch, idx.data(), src, idx.data() + EK, (int32_t)EK, 0)) return rc;
        LaunchRequest req = next_request(scratch);
        req.ep = ep; req.T = H; req.actions = d_x; req.actions_on_device = true;      // (the table policy, no resets, no optional outputs, no time slice)
        req.num_steps = steps_rep.data(); req.done = done_rep.data();
        if (int rc = begin_launch(scratch, req)) return rc;
        if (int rc = run_actions_end_on_device(scratch)) return rc;
        if (int rc = launch_refit(scratch, params, E, d_x, (const ClothStepRecord *)scratch->epi.d_frec, d_s, true, true, false, it == 0)) return rc;
    }
    HIPCHECK(hipMemcpyAsync(mean, P.d_mean, nd, hipMemcpyDeviceToHost, scratch->stream));
    HIPCHECK(hipMemcpyAsync(sdev, P.d_std, nd, hipMemcpyDeviceToHost, scratch->stream));
    HIPCHECK(hipMemcpyAsync(best_actions, P.d_best_a, nd, hipMemcpyDeviceToHost, scratch->stream));
    HIPCHECK(hipMemcpyAsync(best_score, P.d_best_s, (size_t)E * 8, hipMemcpyDeviceToHost, scratch->stream));
    if (scores_out) HIPCHECK(hipMemcpyAsync(scores_out, P.d_scores, ns * n_iters, hipMemcpyDeviceToHost, scratch->stream));
    if (cands_out) HIPCHECK(hipMemcpyAsync(cands_out, P.d_x, nx * n_iters, hipMemcpyDeviceToHost, scratch->stream));
    HIPCHECK(hipStreamSynchronize(scratch->stream));
    return 0;
}
