// api_fit_ddpg.hip -- DDPG on the handle: a Q critic, target networks, the deterministic policy gradient (clothhip.h: DDPG ON THE DEVICE). Host code only: every launch is api_fit.hip's, behind fit_trainer.hpp, and no kernel header is included here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "fit_trainer.hpp"

// Two more loss modes of the trainer (FitLoss::TD, FitLoss::DPG): the TD loss of the Q network, a one-row table as the value network
// is, over dense input rows X = [s, a] that k_fit_concat makes, and the policy's loss -1/B sum Q(s, clamp(mu(s))), whose dZ is the
// critic's input gradient. The Q passes work on their own scratch (Fit::qpass), so the policy's activations survive them. A target copy
// is its network's MlpDesc with params at the target blob: it is only ever passed forward, and has no optimizer.
static_assert(sizeof(ClothDdpgParams) == 24, "ClothDdpgParams is two doubles, a float and an int32");
static_assert(sizeof(ClothBcParams) == 16, "ClothBcParams is two floats and two int32");

static FitNet q_net(clothhip_handle *h) { return {h->qnet.mlp, h->qnet.d_mlp, h->qnet.n_params, 0, h->fit.opt_q, true}; }

// What every DDPG entry refuses of the handle's state; targets: the entry reads or moves the target copies
static int check_ddpg_state(const clothhip_handle *h, bool targets, bool dataset) {
    if (int rc = check_idle(h)) return rc;
    if (h->pol.pop_rows) return fail(CLOTHHIP_ESTATE, "this handle holds a population of networks: DDPG trains the ONE shared network of clothhip_set_policy_mlp");
    if (h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_mlp first");
    if (h->qnet.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no Q network on this handle: call clothhip_set_q_mlp first");
    if (targets && !h->tgt.policy_valid) return fail(CLOTHHIP_ESTATE, "no target policy on this handle (a new policy network drops it): call clothhip_ddpg_sync_targets first");
    if (targets && !h->tgt.q_valid) return fail(CLOTHHIP_ESTATE, "no target Q network on this handle (a new Q network drops it): call clothhip_ddpg_sync_targets first");
    if (dataset && h->dataset.n < 1) return fail(CLOTHHIP_ESTATE, "the dataset is empty: call clothhip_fit_data_append first");
    return 0;
}
static int check_tau(double tau) {
    if (!std::isfinite(tau) || tau < 0.0 || tau > 1.0) return fail(CLOTHHIP_EINVAL, "tau = %g: the soft-update rate is finite and lies in [0, 1]", tau);
    return 0;
}
static int check_ddpg_params(const ClothDdpgParams *q) {
    if (!std::isfinite(q->gamma) || q->gamma < 0.0 || q->gamma > 1.0) return fail(CLOTHHIP_EINVAL, "gamma = %g: the discount is finite and lies in [0, 1]", q->gamma);
    if (int rc = check_tau(q->tau)) return rc;
    if (!(q->act_bound > 0.0f)) return fail(CLOTHHIP_EINVAL, "act_bound = %g: the action bound is > 0 (+inf: no clamp)", (double)q->act_bound);
    if (q->flags) return fail(CLOTHHIP_EINVAL, "unknown flags 0x%x", q->flags);
    return 0;
}
// the minibatches idx [n_idx] of a DDPG call: check_fit_rows, no leaf among them -> succ (may be NULL) [n_idx], the row that holds each
// row's successor state (a terminal row: the row itself, whose value the TD kernel ignores)
static int check_ddpg_rows(const clothhip_handle *h, const int32_t *idx, int64_t n_idx, int32_t B, std::vector<int32_t> *succ) {
    if (int rc = check_fit_rows(h, 1, idx, n_idx, B)) return rc;
    if (succ) { try { succ->resize((size_t)n_idx); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)n_idx); } }
    for (int64_t i = 0; i < n_idx; i++) {
        const int32_t nx = h->dataset.h_next[(size_t)idx[i]];
        if (nx == CLOTHHIP_FIT_NEXT_NONE) return fail(CLOTHHIP_EINVAL, "idx[%lld] = row %d is a leaf: it has no transition (clothhip_fit_data_set_transitions)", (long long)i, idx[i]);
        if (succ) (*succ)[(size_t)i] = nx >= 0 ? nx : idx[i];
    }
    return 0;
}

// DDPG from demonstrations: both coefficients finite and >= 0, not both 0; known flags; reserved 0
static int check_bc_params(const ClothBcParams *bc) {
    if (!std::isfinite(bc->q_coef) || bc->q_coef < 0.0f) return fail(CLOTHHIP_EINVAL, "q_coef = %g: the policy-gradient coefficient is finite and >= 0", (double)bc->q_coef);
    if (!std::isfinite(bc->bc_coef) || bc->bc_coef < 0.0f) return fail(CLOTHHIP_EINVAL, "bc_coef = %g: the behaviour-cloning coefficient is finite and >= 0", (double)bc->bc_coef);
    if (bc->q_coef == 0.0f && bc->bc_coef == 0.0f) return fail(CLOTHHIP_EINVAL, "q_coef and bc_coef are both 0: the step has no loss");
    if (bc->flags & ~CLOTHHIP_BC_QFILTER) return fail(CLOTHHIP_EINVAL, "unknown flags 0x%x", bc->flags);
    if (bc->reserved) return fail(CLOTHHIP_EINVAL, "reserved = %d: must be 0", bc->reserved);
    return 0;
}

enum { DDPG_CRITIC = 1, DDPG_ACTOR = 2, DDPG_POLYAK = 4 };
// Where a DDPG call's results go on the host, each NULL when not wanted: stats [n_steps][3 per network stepped], the critic's first; of
// a gradient call (n_steps 1, nothing updated) the one network's gradient, the critic's y [B] and q [B], the actor's dL/da [B][4]
// ... and of a BC gradient call the actor's dz [B][4] and the critic on the expert's action qe [B]
struct DdpgOut { double *stats; float *grad, *y, *q, *da, *dz, *qe; };

// n_steps steps over idx [n_steps][B] (succ beside it, for the critic): per step the critic's (DDPG_CRITIC), the actor's against the
// critic as it stands then (DDPG_ACTOR), the soft update of both targets (DDPG_POLYAK); update false: the gradients only. The call is valid.
// bc (NULL: plain DDPG, k_fit_dpg_dz): the actor's step is that of DDPG from demonstrations, k_fit_dpg_bc in the place of k_fit_dpg_dz,
// and under the Q-filter the live critic is first passed over [s, clamp(a_E)] -- into the SECOND activation slot of the Q passes, the
// target critic's of the critic's step, free here -- with input rows of its own (d_qxe).
static int run_ddpg(clothhip_handle *h, int mode, bool update, const ClothFitParams *p_policy, const ClothFitParams *p_q, const ClothDdpgParams &q, const int32_t *idx,
                    const int32_t *succ, int32_t n_steps, int32_t B, const DdpgOut &out, const ClothBcParams *bc = nullptr) {
    auto &f = h->fit;
    const bool critic = (mode & DDPG_CRITIC) != 0, actor = (mode & DDPG_ACTOR) != 0;
    const bool filter = bc && (bc->flags & CLOTHHIP_BC_QFILTER);
    const FitNet pnet = policy_net(h), qnet = q_net(h);
    MlpDesc tp_desc = h->pol.mlp, tq_desc = h->qnet.mlp;      // the target copies
    tp_desc.params = h->tgt.d_policy; tq_desc.params = h->tgt.d_q;
    const FitPlan pp = fit_plan(pnet.D, B), qp = fit_plan(qnet.D, B);
    const int Lp = pnet.D.n_layers, Lq = qnet.D.n_layers;
    const size_t n_rows = (size_t)n_steps * B, xw = (size_t)3 * h->P + MLP_OUT;
    // the step constants of both optimizers, the critic's table first; nothing of the handle changes yet
    OptPlan opt;
    int k_critic = -1, k_actor = -1;
    if (update && critic) { k_critic = opt.n; opt.add(net_target(qnet, SHARED_ROW, 1, f.qpass.d_grad, p_q)); }
    if (update && actor) { k_actor = opt.n; opt.add(net_target(pnet, SHARED_ROW, 1, f.own.d_grad, p_policy)); }
    if (int rc = opt_prepare(opt, n_steps)) return rc;
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = fit_reserve(h, pp, 1)) return rc;
    if (int rc = f.d_qx.reserve((size_t)B * xw * 4)) return rc;
    if (filter) if (int rc = f.d_qxe.reserve((size_t)B * xw * 4)) return rc;
    if (int rc = fit_reserve(f.qpass, qp, 1, 2)) return rc;      // (activations: the live critic's, then the target's)
    if (int rc = f.d_da.reserve((size_t)B * MLP_OUT * 4)) return rc;
    if (int rc = f.d_tdy.reserve((size_t)B * 4)) return rc;
    if (int rc = f.d_idx.reserve(n_rows * 4)) return rc;
    if (critic) if (int rc = f.d_succ.reserve(n_rows * 4)) return rc;
    const FitWork pw = fit_work(f.own), qw = fit_work(f.qpass, f.d_qx);
    const FitWork tqw = {qw.act + qp.act, nullptr, nullptr, nullptr, qw.x};      // the second network's worth of activations: a forward alone
    const float *qv = qw.act + qp.h_off[Lq - 1], *y = pw.act + pp.h_off[Lp - 1];
    const FitWork eqw = {tqw.act, nullptr, nullptr, nullptr, f.d_qxe};      // ... the live critic on the expert's action, in that slot
    const float *qe = tqw.act + qp.h_off[Lq - 1];
    const FitLoss td = td_loss(tqw.act + qp.h_off[Lq - 1], f.d_tdy, q.gamma);
    const FitLoss dpg = bc ? dpg_bc_loss(f.d_da, qv, filter ? qe : nullptr, q.act_bound, bc->q_coef, bc->bc_coef) : dpg_loss(f.d_da, qv, q.act_bound);
    const int n_stats = (critic ? td.stats : 0) + (actor ? dpg.stats : 0);
    if (int rc = f.d_loss.reserve((size_t)n_steps * n_stats * 8)) return rc;
    if (int rc = opt_reserve(h, opt)) return rc;
    // from here on the call goes through (but for a failure of the runtime itself)
    if (int rc = opt_commit(h, opt)) return rc;
    HIPCHECK(hipMemcpyAsync(f.d_members, SHARED_ROW, 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_idx, idx, n_rows * 4, hipMemcpyHostToDevice, h->stream));
    if (critic) HIPCHECK(hipMemcpyAsync(f.d_succ, succ, n_rows * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    float *q_dz = qw.dz + ((Lq - 1) & 1) * (size_t)B * qp.maxw;
    const float seed_f = -1.0f / (float)B;      // the dZ of the critic's last layer under L = -1/B sum Q
    int seed_bits;
    memcpy(&seed_bits, &seed_f, 4);
    for (int s = 0; s < n_steps; s++) {
        const int32_t *d_idx = f.d_idx + (size_t)s * B, *d_succ = f.d_succ + (size_t)s * B;
        double *st = f.d_loss + (size_t)s * n_stats;
        if (critic) {
            // the target critic on [s', clamp(mu'(s'))]: the target policy over the successor rows, on the policy's scratch
            if (int rc = enqueue_forward(h, tp_desc, pp, 1, d_succ, B, false, pw)) return rc;
            if (int rc = enqueue_concat(h, false, y, d_succ, B, q.act_bound)) return rc;
            if (int rc = enqueue_forward(h, tq_desc, qp, 1, nullptr, B, false, tqw)) return rc;
            // the critic on [s, clamp(a)], a the action the row executed
            if (int rc = enqueue_concat(h, true, nullptr, d_idx, B, q.act_bound)) return rc;
            if (int rc = enqueue_forward(h, qnet.D, qp, 1, nullptr, B, false, qw)) return rc;
            if (int rc = enqueue_loss(h, qnet, qp, td, 1, d_idx, B, st, nullptr, nullptr, qw)) return rc;
            if (int rc = enqueue_backward(h, qnet.D, qp, 1, nullptr, B, qw)) return rc;
            if (update) if (int rc = enqueue_optimizer(h, opt, k_critic, s)) return rc;
            st += td.stats;
        }
        if (actor) {
            if (filter) {
                if (int rc = enqueue_concat_expert(h, d_idx, B, q.act_bound)) return rc;
                if (int rc = enqueue_forward(h, qnet.D, qp, 1, nullptr, B, false, eqw)) return rc;
            }
            if (int rc = enqueue_forward(h, pnet.D, pp, 1, d_idx, B, false, pw)) return rc;
            if (int rc = enqueue_concat(h, false, y, d_idx, B, q.act_bound)) return rc;
            if (int rc = enqueue_forward(h, qnet.D, qp, 1, nullptr, B, false, qw)) return rc;
            HIPCHECK(hipMemsetD32Async((hipDeviceptr_t)q_dz, seed_bits, (size_t)B, h->stream));
            if (int rc = enqueue_action_grad(h, qnet.D, qp, B, qw)) return rc;
            if (int rc = enqueue_loss(h, pnet, pp, dpg, 1, d_idx, B, st, nullptr, nullptr, pw)) return rc;
            // (a gradient call's dz goes out here, in stream order: the backward pass reuses the table for the dZ two layers down)
            if (out.dz) HIPCHECK(hipMemcpyAsync(out.dz, pw.dz + ((Lp - 1) & 1) * (size_t)B * pp.maxw, (size_t)B * MLP_OUT * 4, hipMemcpyDeviceToHost, h->stream));
            if (int rc = enqueue_backward(h, pnet.D, pp, 1, d_idx, B, pw)) return rc;
            if (update) if (int rc = enqueue_optimizer(h, opt, k_actor, s)) return rc;
        }
        if (mode & DDPG_POLYAK) if (int rc = enqueue_polyak(h, q.tau)) return rc;
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    f.ddpg_x_expert = actor && filter;
    f.ddpg_B = B; f.ddpg_critic = critic && !(actor && filter); f.ddpg_qn_at = qp.act + qp.h_off[Lq - 1]; f.ddpg_q_at = qp.h_off[Lq - 1];
    if (out.stats) HIPCHECK(hipMemcpyAsync(out.stats, f.d_loss, (size_t)n_steps * n_stats * 8, hipMemcpyDeviceToHost, h->stream));
    if (out.grad) HIPCHECK(hipMemcpyAsync(out.grad, critic ? qw.grad : pw.grad, (critic ? qp.grad : pp.grad) * 4, hipMemcpyDeviceToHost, h->stream));
    if (out.y) HIPCHECK(hipMemcpyAsync(out.y, f.d_tdy, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (out.q) HIPCHECK(hipMemcpyAsync(out.q, qv, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (out.da) HIPCHECK(hipMemcpyAsync(out.da, f.d_da, (size_t)B * MLP_OUT * 4, hipMemcpyDeviceToHost, h->stream));
    if (out.qe) HIPCHECK(hipMemcpyAsync(out.qe, qe, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));      // (the host tables are never retained)
    return 0;
}

extern "C" int clothhip_q_fit_grad(clothhip_handle *h, const ClothDdpgParams *q, const int32_t *idx, int32_t B, float *grad_out, double *stats_out, float *y_out,
                                   float *q_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_ddpg_state(h, true, true)) return rc;
    std::vector<int32_t> succ;
    if (int rc = check_ddpg_rows(h, idx, B, B, &succ)) return rc;
    if (int rc = check_ddpg_params(q)) return rc;
    return run_ddpg(h, DDPG_CRITIC, false, nullptr, nullptr, *q, idx, succ.data(), 1, B, {stats_out, grad_out, y_out, q_out, nullptr});
}

extern "C" int clothhip_policy_fit_dpg_grad(clothhip_handle *h, const ClothDdpgParams *q, const int32_t *idx, int32_t B, float *grad_out, double *stats_out,
                                            float *da_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_ddpg_state(h, false, true)) return rc;
    if (int rc = check_ddpg_rows(h, idx, B, B, nullptr)) return rc;
    if (int rc = check_ddpg_params(q)) return rc;
    return run_ddpg(h, DDPG_ACTOR, false, nullptr, nullptr, *q, idx, nullptr, 1, B, {stats_out, grad_out, nullptr, nullptr, da_out});
}

// the step entries behind their argument lists: p_policy / p_q NULL where the mode does not train that network; with_bc: the actor's
// step is that of DDPG from demonstrations under bc
static int ddpg_steps(clothhip_handle *h, int mode, const ClothFitParams *p_policy, const ClothFitParams *p_q, const ClothDdpgParams *q, const int32_t *idx,
                      int32_t n_steps, int32_t B, double *stats_out, bool with_bc = false, const ClothBcParams *bc = nullptr) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!q || ((mode & DDPG_ACTOR) && !p_policy) || ((mode & DDPG_CRITIC) && !p_q) || (with_bc && !bc)) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_ddpg_state(h, mode != DDPG_ACTOR, true)) return rc;
    std::vector<int32_t> succ;
    if (int rc = check_ddpg_rows(h, idx, (int64_t)n_steps * B, B, (mode & DDPG_CRITIC) ? &succ : nullptr)) return rc;
    if (mode & DDPG_ACTOR) if (int rc = check_fit_params(p_policy, -1)) return rc;
    if (mode & DDPG_CRITIC) if (int rc = check_fit_params(p_q, -1)) return rc;
    if (int rc = check_ddpg_params(q)) return rc;
    if (with_bc) if (int rc = check_bc_params(bc)) return rc;
    if (n_steps == 0) return 0;
    return run_ddpg(h, mode, true, p_policy, p_q, *q, idx, succ.data(), n_steps, B, {stats_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, bc);
}

extern "C" int clothhip_q_fit(clothhip_handle *h, const ClothFitParams *p, const ClothDdpgParams *q, const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out) {
    return ddpg_steps(h, DDPG_CRITIC, nullptr, p, q, idx, n_steps, B, stats_out);
}

extern "C" int clothhip_policy_fit_dpg(clothhip_handle *h, const ClothFitParams *p, const ClothDdpgParams *q, const int32_t *idx, int32_t n_steps, int32_t B,
                                       double *stats_out) {
    return ddpg_steps(h, DDPG_ACTOR, p, nullptr, q, idx, n_steps, B, stats_out);
}

extern "C" int clothhip_ddpg_fit(clothhip_handle *h, const ClothFitParams *p_policy, const ClothFitParams *p_q, const ClothDdpgParams *q, const int32_t *idx,
                                 int32_t n_steps, int32_t B, double *stats_out) {
    return ddpg_steps(h, DDPG_CRITIC | DDPG_ACTOR | DDPG_POLYAK, p_policy, p_q, q, idx, n_steps, B, stats_out);
}

// ---- DDPG from demonstrations (clothhip.h: DDPG FROM DEMONSTRATIONS): the actor's step with a behaviour-cloning term -------------------------
extern "C" int clothhip_policy_fit_dpg_bc_grad(clothhip_handle *h, const ClothDdpgParams *q, const ClothBcParams *bc, const int32_t *idx, int32_t B, float *grad_out,
                                               double *stats_out, float *da_out, float *dz_out, float *q_out, float *qe_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!q || !bc) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_ddpg_state(h, false, true)) return rc;
    if (int rc = check_ddpg_rows(h, idx, B, B, nullptr)) return rc;
    if (int rc = check_ddpg_params(q)) return rc;
    if (int rc = check_bc_params(bc)) return rc;
    if (qe_out && !(bc->flags & CLOTHHIP_BC_QFILTER)) return fail(CLOTHHIP_EINVAL, "qe_out without CLOTHHIP_BC_QFILTER: the critic is not passed over the expert's action");
    return run_ddpg(h, DDPG_ACTOR, false, nullptr, nullptr, *q, idx, nullptr, 1, B, {stats_out, grad_out, nullptr, q_out, da_out, dz_out, qe_out}, bc);
}

extern "C" int clothhip_policy_fit_dpg_bc(clothhip_handle *h, const ClothFitParams *p, const ClothDdpgParams *q, const ClothBcParams *bc, const int32_t *idx,
                                          int32_t n_steps, int32_t B, double *stats_out) {
    return ddpg_steps(h, DDPG_ACTOR, p, nullptr, q, idx, n_steps, B, stats_out, true, bc);
}

extern "C" int clothhip_ddpg_fit_bc(clothhip_handle *h, const ClothFitParams *p_policy, const ClothFitParams *p_q, const ClothDdpgParams *q, const ClothBcParams *bc,
                                    const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out) {
    return ddpg_steps(h, DDPG_CRITIC | DDPG_ACTOR | DDPG_POLYAK, p_policy, p_q, q, idx, n_steps, B, stats_out, true, bc);
}

extern "C" int clothhip_ddpg_polyak(clothhip_handle *h, double tau) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_ddpg_state(h, true, false)) return rc;
    if (int rc = check_tau(tau)) return rc;
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    if (int rc = enqueue_polyak(h, tau)) return rc;
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// what the last DDPG call left in the Q passes' scratch (clothhip.h: for tests of the elementwise kernels)
extern "C" int clothhip_ddpg_last_tables(clothhip_handle *h, int32_t B, float *x_out, float *qn_out, float *q_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    auto &f = h->fit;
    if (f.ddpg_B < 1) return fail(CLOTHHIP_ESTATE, "no DDPG call has run on this handle's present Q network");
    if (B != f.ddpg_B) return fail(CLOTHHIP_EINVAL, "B = %d, the last DDPG call ran minibatches of %d rows", B, f.ddpg_B);
    if (qn_out && !f.ddpg_critic) return fail(CLOTHHIP_ESTATE, "the last DDPG call ran no critic's step: there are no target critic's values");
    HIPCHECK(hipSetDevice(h->device));
    if (x_out) HIPCHECK(hipMemcpyAsync(x_out, f.ddpg_x_expert ? f.d_qxe : f.d_qx, (size_t)B * ((size_t)3 * h->P + MLP_OUT) * 4, hipMemcpyDeviceToHost, h->stream));
    if (qn_out) HIPCHECK(hipMemcpyAsync(qn_out, f.qpass.d_act + f.ddpg_qn_at, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (q_out) HIPCHECK(hipMemcpyAsync(q_out, f.qpass.d_act + f.ddpg_q_at, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_q_fit_reset(clothhip_handle *h) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    h->fit.opt_q.forget();
    return 0;
}
