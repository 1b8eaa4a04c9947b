// api_fit.hip -- the trainer of the handle's networks, policy, critic and Q critic, over the dataset of api_fit_data.hip (fit_trainer.hpp has its types): every launch of a step -- forward, the losses, backward, the optimizers --, the optimizer's bookkeeping across calls, and the supervised, PPO (fixed or learned sigma, shared network or population rows under their own constants) and value entries. The one includer of cloth_policy_fit.hpp and cloth_fit_ddpg.hpp: api_fit_rollout.hip and api_fit_ddpg.hip launch through the functions here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <vector>

#include "cloth_fit_ddpg.hpp"
#include "cloth_policy_fit.hpp"
#include "fit_trainer.hpp"

static_assert(FIT_MAX_BATCH == CLOTHHIP_FIT_MAX_BATCH, "the batch cap of the header and of the kernels");
static_assert(sizeof(ClothFitParams) == 24, "ClothFitParams is six floats");

// ---- the trainer (cloth_policy_fit.hpp has the definition and the order) ----------------------------------------------------------------
// ONE path: a call fits n_m rows of the handle's weight table in the launches of one network. The table is the population d_pop
// [pop_rows][mlp.stride], or the shared network d_mlp as a table of one row: the shared entries are the call members = {0}, n_m = 1 (row
// 0 lies at offset 0 whatever mlp.stride holds). The extern "C" entries below only refuse what each of them refuses and call it.
static_assert(CLOTHHIP_FIT_MAX_MEMBER_ROWS == 65536, "the header's cap on n_m * B of one call");

const int32_t SHARED_ROW[1] = {0};

FitNet policy_net(clothhip_handle *h) {
    return {h->pol.mlp, h->pol.pop_rows ? h->pol.d_pop : h->pol.d_mlp, h->pol.mlp_n_params, h->pol.pop_rows, h->fit.opt_policy, false};
}
FitNet value_net(clothhip_handle *h) { return {h->val.mlp, h->val.d_mlp, h->val.n_params, 0, h->fit.opt_value, true}; }

// What the entries refuse before anything is touched, each in the order it always had. The state; `population`: the entry trains rows of
// a population (which puts these refusals first, whatever else is wrong with the call), else the shared network
int check_fit_state(const clothhip_handle *h, bool population) {
    if (int rc = check_idle(h)) return rc;
    if (population) {
        if (h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_population first");
        if (!h->pol.pop_rows) return fail(CLOTHHIP_ESTATE, "this handle holds ONE shared network, not a population: use clothhip_policy_fit");
    } else {
        if (h->pol.pop_rows) return fail(CLOTHHIP_ESTATE, "this handle holds a population of networks: the fit trains the ONE shared network of clothhip_set_policy_mlp");
        if (h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_mlp first");
    }
    if (h->dataset.n < 1) return fail(CLOTHHIP_ESTATE, "the dataset is empty: call clothhip_fit_data_append first");
    return 0;
}
// ... and of the entries that train or evaluate the value network (a population is no obstacle: the critic is not the policy)
int check_value_state(const clothhip_handle *h) {
    if (int rc = check_idle(h)) return rc;
    if (h->val.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no value network on this handle: call clothhip_set_value_mlp first");
    if (h->dataset.n < 1) return fail(CLOTHHIP_ESTATE, "the dataset is empty: call clothhip_fit_data_append first");
    return 0;
}
// the member list of a call ...
static int check_fit_members(const clothhip_handle *h, const int32_t *members, int32_t n_m) {
    if (n_m < 1) return fail(CLOTHHIP_EINVAL, "n_m = %d: a call names at least one member", n_m);
    if (!members) return fail(CLOTHHIP_EINVAL, "members is NULL");
    std::vector<uint8_t> seen;
    try { seen.assign((size_t)h->pol.pop_rows, 0); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)h->pol.pop_rows); }
    for (int32_t j = 0; j < n_m; j++) {
        if (members[j] < 0 || members[j] >= h->pol.pop_rows)
            return fail(CLOTHHIP_EINVAL, "members[%d] = %d outside [0, %lld)", j, members[j], (long long)h->pol.pop_rows);
        if (seen[members[j]]) return fail(CLOTHHIP_EINVAL, "members[%d] = %d is named twice: a call fits a row once", j, members[j]);
        seen[members[j]] = 1;
    }
    return 0;
}
// ... its minibatches: n_idx entries of idx in all, B rows per member and step ...
int check_fit_rows(const clothhip_handle *h, int32_t n_m, const int32_t *idx, int64_t n_idx, int32_t B) {
    if (B < 1 || B > FIT_MAX_BATCH) return fail(CLOTHHIP_EINVAL, "B = %d outside [1, %d]", B, FIT_MAX_BATCH);
    if ((int64_t)n_m * B > CLOTHHIP_FIT_MAX_MEMBER_ROWS)
        return fail(CLOTHHIP_EINVAL, "n_m * B = %d * %d rows in one call, at most %d", n_m, B, CLOTHHIP_FIT_MAX_MEMBER_ROWS);
    if (!idx && n_idx > 0) return fail(CLOTHHIP_EINVAL, "idx is NULL");
    for (int64_t i = 0; i < n_idx; i++)
        if (idx[i] < 0 || idx[i] >= h->dataset.n) return fail(CLOTHHIP_EINVAL, "idx[%lld] = %d outside [0, %lld)", (long long)i, idx[i], (long long)h->dataset.n);
    return 0;
}
// ... and the optimizer of member j (j < 0: the one of the shared network, named without an index)
static bool hyper_ok(float v) { return std::isfinite(v) && v >= 0.0f; }
int check_fit_params(const ClothFitParams *p, int32_t j) {
    char who[24] = "";
    if (j >= 0) snprintf(who, sizeof(who), "p[%d]: ", j);
    if (p->optimizer != (float)CLOTHHIP_FIT_ADAM && p->optimizer != (float)CLOTHHIP_FIT_SGD)
        return fail(CLOTHHIP_EINVAL, "%sunknown optimizer %g (CLOTHHIP_FIT_ADAM or CLOTHHIP_FIT_SGD)", who, (double)p->optimizer);
    if (!hyper_ok(p->lr) || !hyper_ok(p->eps) || !hyper_ok(p->momentum) || !hyper_ok(p->beta1) || !hyper_ok(p->beta2))
        return fail(CLOTHHIP_EINVAL, "%sa hyper-parameter is negative or not finite (lr %g, beta1 %g, beta2 %g, eps %g, momentum %g)", who, (double)p->lr,
                    (double)p->beta1, (double)p->beta2, (double)p->eps, (double)p->momentum);
    if (p->beta1 >= 1.0f || p->beta2 >= 1.0f) return fail(CLOTHHIP_EINVAL, "%sbeta1 %g, beta2 %g: both lie in [0, 1)", who, (double)p->beta1, (double)p->beta2);
    return 0;
}

// ... and the optimizers p [n_m] of a grouped step entry: each valid by its index, and one optimizer per call
static int check_fit_params_members(const ClothFitParams *p, int32_t n_m) {
    for (int32_t j = 0; j < n_m; j++) {
        if (int rc = check_fit_params(p + j, j)) return rc;
        if (p[j].optimizer != p[0].optimizer) return fail(CLOTHHIP_EINVAL, "p[%d].optimizer = %g, p[0].optimizer = %g: one optimizer per call", j, (double)p[j].optimizer, (double)p[0].optimizer);
    }
    return 0;
}

// Where member j's tables lie (FitPlan): the sizes for minibatches of B rows and the offsets of every layer of D
FitPlan fit_plan(const MlpDesc &D, int32_t B) {
    FitPlan p = {};
    size_t maxmat = 0;
    p.maxw = MLP_OUT;
    for (int l = 0; l < D.n_layers; l++) {
        p.w_off[l] = p.grad; p.h_off[l] = p.act;
        p.grad += (size_t)D.widths[l + 1] * D.widths[l] + D.widths[l + 1];
        p.act += (size_t)B * D.widths[l + 1];
        p.maxw = std::max<size_t>(p.maxw, D.widths[l + 1]);
        maxmat = std::max<size_t>(maxmat, (size_t)D.widths[l + 1] * D.widths[l]);
    }
    p.dz = 2 * (size_t)B * p.maxw;
    p.n_split = (B + FIT_SPLIT_ROWS - 1) / FIT_SPLIT_ROWS;
    p.part = p.n_split > 1 ? (size_t)p.n_split * maxmat : 0;
    return p;
}
// one step's scratch in t: n_grad members' dZ tables, slabs and gradients, n_act passes' activations
int fit_reserve(clothhip_handle::Fit::Pass &t, const FitPlan &p, size_t n_grad, size_t n_act) {
    if (int rc = t.d_act.reserve(n_act * p.act * 4)) return rc;
    if (int rc = t.d_dz.reserve(n_grad * p.dz * 4)) return rc;
    if (p.part) if (int rc = t.d_part.reserve(n_grad * p.part * 4)) return rc;
    return t.d_grad.reserve(n_grad * p.grad * 4);
}
// ... the trainer's own for n_m members, and the call's member table
int fit_reserve(clothhip_handle *h, const FitPlan &p, int32_t n_m) {
    if (int rc = h->fit.d_members.reserve((size_t)n_m * 4)) return rc;
    return fit_reserve(h->fit.own, p, (size_t)n_m, (size_t)n_m);
}
// the ONE place a FitWork is made from an instance (valid after its fit_reserve)
FitWork fit_work(const clothhip_handle::Fit::Pass &t, const float *x) { return {t.d_act, t.d_dz, t.d_part, t.d_grad, x}; }

template <bool A_KC, bool B_KC, int EPI, bool ROWS> static void launch_gemm(hipStream_t s, FitGemmArgs &a, int32_t n_m) {
    a.tiles_n = (a.N + FIT_TILE - 1) / FIT_TILE;
    const dim3 grid((unsigned)a.tiles_n * (unsigned)n_m, (unsigned)((a.M + FIT_TILE - 1) / FIT_TILE), (unsigned)((a.K + a.k_chunk - 1) / a.k_chunk));
    hipLaunchKernelGGL((k_fit_gemm<A_KC, B_KC, EPI, ROWS>), grid, dim3(FIT_THREADS), 0, s, a);
}

// the losses (FitLoss: fit_trainer.hpp), each with the statistics its kernel writes
static FitLoss squared_error() { FitLoss l = {}; l.kind = FitLoss::SQUARED_ERROR; l.stats = 1; return l; }
static FitLoss ppo_loss(const double *q) { FitLoss l = {}; l.kind = FitLoss::PPO; l.stats = FIT_PPO_STATS; l.q = q; return l; }
static FitLoss ppo_sigma_loss(double lo, double hi, double ent_coef) { FitLoss l = {}; l.kind = FitLoss::PPO_SIGMA; l.stats = FIT_PPO_SIGMA_STATS; l.s = {lo, hi, ent_coef}; return l; }
FitLoss td_loss(const float *qn, float *y_out, double gamma) { FitLoss l = {}; l.kind = FitLoss::TD; l.stats = FIT_TD_STATS; l.td = {qn, y_out, gamma}; return l; }
FitLoss dpg_loss(const float *dA, const float *q, float bound) { FitLoss l = {}; l.kind = FitLoss::DPG; l.stats = FIT_DPG_STATS; l.dpg = {dA, q, bound}; return l; }
FitLoss dpg_bc_loss(const float *dA, const float *q, const float *qe, float bound, float qc, float bc) {
    FitLoss l = {}; l.kind = FitLoss::DPG_BC; l.stats = FIT_DPG_BC_STATS; l.bc = {dA, q, qe, bound, qc, bc}; return l;
}

// The launches of one network's step, each over all n_m members: forward, loss, backward. The forward of the present weights over rows
// d_idx [n_m][B]: member j's y is then at w.act + j * p.act + p.h_off[L - 1].
// shared_rows: d_idx is ONE list [B] that every member reads
int enqueue_forward(clothhip_handle *h, const MlpDesc &D, const FitPlan &p, int32_t n_m, const int32_t *d_idx, int32_t B, bool shared_rows,
                           const FitWork &w) {
    const int L = D.n_layers;
    float *act = w.act;
    FitGemmArgs m0 = {};
    m0.members = h->fit.d_members; m0.stride = D.stride; m0.rows_step = shared_rows ? 0 : B;
    for (int l = 0; l < L; l++) {
        const int n_in = D.widths[l], n_out = D.widths[l + 1];
        FitGemmArgs a = m0;
        const bool gather = l == 0 && !w.x;      // layer 0 reads the dataset through the index table, unless the pass has its own input rows
        a.A = l ? act + p.h_off[l - 1] : gather ? (const float *)h->dataset.obs() : w.x; a.lda = n_in; a.rows = gather ? d_idx : nullptr; a.a_step = l ? (int64_t)p.act : 0;
        a.B = D.params + p.w_off[l]; a.ldb = n_in; a.bias = a.B + (size_t)n_out * n_in; a.b_weights = 1;
        a.C = act + p.h_off[l]; a.ldc = n_out; a.c_step = (int64_t)p.act;
        a.M = B; a.N = n_out; a.K = n_in; a.k_chunk = n_in;
        if (gather && l + 1 < L) launch_gemm<true, true, FIT_EPI_BIAS_RELU, true>(h->stream, a, n_m);
        else if (gather) launch_gemm<true, true, FIT_EPI_BIAS, true>(h->stream, a, n_m);
        else if (l + 1 < L) launch_gemm<true, true, FIT_EPI_BIAS_RELU, false>(h->stream, a, n_m);
        else launch_gemm<true, true, FIT_EPI_BIAS, false>(h->stream, a, n_m);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}
// The loss of the forward's y in w and its dZ of the last layer, into w: d_stats [n_m][loss.stats]. The surrogates: d_ratio (may be NULL)
// [n_m][B]; PPO reads member j's constants from row j of h->fit.d_ppo_q (the caller has uploaded loss.q); PPO_SIGMA reads the handle's
// log-sigma head where it lies, writes the head's gradient to h->fit.d_grad_ls and the head it read to d_ls (may be NULL). TD, DPG and DPG_BC
// (n_m == 1): cloth_fit_ddpg.hpp's one workgroup each
int enqueue_loss(clothhip_handle *h, const FitNet &net, const FitPlan &p, const FitLoss &loss, int32_t n_m, const int32_t *d_idx, int32_t B, double *d_stats,
                        float *d_ratio, float *d_ls, const FitWork &w) {
    auto &f = h->fit;
    const auto &d = h->dataset;
    const int L = net.D.n_layers;
    const float *y = w.act + p.h_off[L - 1];
    float *dz = w.dz + ((L - 1) & 1) * (size_t)B * p.maxw;
    const dim3 grid((unsigned)n_m), block(256);
    if (loss.kind == FitLoss::TD) {
        FitTdArgs t = {};
        t.q = y; t.qn = loss.td.qn; t.rew = d.rew(); t.next = d.next(); t.rows = d_idx; t.dz = dz; t.y_out = loss.td.y_out; t.stats = d_stats;
        t.gamma = loss.td.gamma; t.B = B;
        hipLaunchKernelGGL(k_fit_loss_td, dim3(1), dim3(FIT_DDPG_THREADS), 0, h->stream, t);
    } else if (loss.kind == FitLoss::DPG) {
        FitDpgArgs g = {};
        g.dA = loss.dpg.dA; g.y = y; g.q = loss.dpg.q; g.dz = dz; g.stats = d_stats; g.bound = loss.dpg.bound; g.B = B;
        hipLaunchKernelGGL(k_fit_dpg_dz, dim3(1), dim3(FIT_DDPG_THREADS), 0, h->stream, g);
    } else if (loss.kind == FitLoss::DPG_BC) {
        FitDpgBcArgs g = {};
        g.dA = loss.bc.dA; g.y = y; g.q = loss.bc.q; g.qe = loss.bc.qe; g.expert = d.expert(); g.rows = d_idx; g.dz = dz; g.stats = d_stats;
        g.bound = loss.bc.bound; g.qc = loss.bc.qc; g.bc = loss.bc.bc; g.B = B;
        hipLaunchKernelGGL(k_fit_dpg_bc, dim3(1), dim3(FIT_DDPG_THREADS), 0, h->stream, g);
    } else if (loss.kind == FitLoss::PPO_SIGMA) {
        FitPpoSigmaArgs q = {};
        q.y = y; q.lab = d.lab(); q.old = d.old(); q.old_ls = d.old_ls(); q.wgt = d.w(); q.ls = h->pol.d_log_sigma; q.rows = d_idx;
        q.dz = dz; q.ratio = d_ratio; q.grad_ls = f.d_grad_ls; q.ls_out = d_ls; q.stats = d_stats;
        q.lo = loss.s.lo; q.hi = loss.s.hi; q.ent_coef = loss.s.ent_coef;
        q.y_step = (int64_t)p.act; q.dz_step = (int64_t)p.dz; q.rows_step = (int64_t)B; q.B = B;
        hipLaunchKernelGGL(k_fit_loss_ppo_sigma, grid, block, 0, h->stream, q);
    } else if (loss.kind == FitLoss::PPO) {
        FitPpoArgs q = {};
        q.y = y; q.lab = d.lab(); q.old = d.old(); q.wgt = d.w(); q.rows = d_idx; q.dz = dz; q.ratio = d_ratio; q.stats = d_stats; q.q = f.d_ppo_q;
        q.y_step = (int64_t)p.act; q.dz_step = (int64_t)p.dz; q.rows_step = (int64_t)B; q.B = B;
        hipLaunchKernelGGL(k_fit_loss_ppo, grid, block, 0, h->stream, q);
    } else if (net.value)      // SQUARED_ERROR, at the net's width
        hipLaunchKernelGGL(k_fit_loss<1>, grid, block, 0, h->stream, y, (const float *)d.ret(), (const float *)nullptr, d_idx, B, dz, d_stats, (int64_t)p.act, (int64_t)p.dz, (int64_t)B);
    else
        hipLaunchKernelGGL(k_fit_loss<4>, grid, block, 0, h->stream, y, (const float *)d.lab(), (const float *)d.w(), d_idx, B, dz, d_stats, (int64_t)p.act, (int64_t)p.dz, (int64_t)B);
    HIPCHECK(hipGetLastError());
    return 0;
}
// dZ_{l-1} = mask(dZ_l W_l), l > 0, of every member: the input gradient of layer l under the ReLU mask of layer l - 1's activations
static int enqueue_input_grad(clothhip_handle *h, const MlpDesc &D, const FitPlan &p, int l, int32_t n_m, int32_t B, const FitWork &w) {
    const int n_in = D.widths[l], n_out = D.widths[l + 1];
    float *dz[2] = {w.dz, w.dz + (size_t)B * p.maxw};
    FitGemmArgs b = {};
    b.members = h->fit.d_members; b.stride = D.stride; b.rows_step = B;
    b.A = dz[l & 1]; b.lda = n_out; b.a_step = (int64_t)p.dz;
    b.B = D.params + p.w_off[l]; b.ldb = n_in; b.b_weights = 1;
    b.mask = w.act + p.h_off[l - 1]; b.mask_step = (int64_t)p.act;
    b.C = dz[(l - 1) & 1]; b.ldc = n_in; b.c_step = (int64_t)p.dz;
    b.M = B; b.N = n_in; b.K = n_out; b.k_chunk = n_out;
    launch_gemm<true, false, FIT_EPI_MASK, false>(h->stream, b, n_m);
    HIPCHECK(hipGetLastError());
    return 0;
}
// The backward from the loss launch's dZ: the gradient of every member into w.grad [n_m][n_params] (blob layout)
int enqueue_backward(clothhip_handle *h, const MlpDesc &D, const FitPlan &p, int32_t n_m, const int32_t *d_idx, int32_t B, const FitWork &w) {
    auto &f = h->fit;
    float *act = w.act, *grad = w.grad, *dz[2] = {w.dz, w.dz + (size_t)B * p.maxw};
    FitGemmArgs m0 = {};
    m0.members = f.d_members; m0.stride = D.stride; m0.rows_step = B;
    for (int l = D.n_layers - 1; l >= 0; l--) {
        const int n_in = D.widths[l], n_out = D.widths[l + 1];
        const float *dzl = dz[l & 1];
        float *gWl = grad + p.w_off[l];
        FitGemmArgs a = m0;
        a.A = dzl; a.lda = n_out; a.a_step = (int64_t)p.dz;
        const bool gather = l == 0 && !w.x;
        a.B = l ? act + p.h_off[l - 1] : gather ? (const float *)h->dataset.obs() : w.x; a.ldb = n_in; a.rows = gather ? d_idx : nullptr; a.b_step = l ? (int64_t)p.act : 0;
        a.C = p.n_split > 1 ? w.part : gWl; a.ldc = n_in; a.c_slab = (int64_t)n_out * n_in; a.c_step = (int64_t)(p.n_split > 1 ? p.part : p.grad);
        a.M = n_out; a.N = n_in; a.K = B; a.k_chunk = FIT_SPLIT_ROWS;
        if (gather) launch_gemm<false, false, FIT_EPI_NONE, true>(h->stream, a, n_m);
        else launch_gemm<false, false, FIT_EPI_NONE, false>(h->stream, a, n_m);
        HIPCHECK(hipGetLastError());
        if (p.n_split > 1) {
            const int64_t n = (int64_t)n_out * n_in;
            const int32_t blocks = (int32_t)((n + 255) / 256);
            hipLaunchKernelGGL(k_fit_reduce, dim3((unsigned)blocks * (unsigned)n_m), dim3(256), 0, h->stream, (const float *)w.part, n, p.n_split, gWl, n,
                               (int64_t)p.part, (int64_t)p.grad, blocks);
            HIPCHECK(hipGetLastError());
        }
        const int32_t cblocks = (n_out + 63) / 64;
        hipLaunchKernelGGL(k_fit_colsum, dim3((unsigned)cblocks * (unsigned)n_m), dim3(64), 0, h->stream, dzl, B, n_out, gWl + (size_t)n_out * n_in,
                           (int64_t)p.dz, (int64_t)p.grad, cblocks);
        HIPCHECK(hipGetLastError());
        if (l > 0) if (int rc = enqueue_input_grad(h, D, p, l, n_m, B, w)) return rc;
    }
    return 0;
}
// ... and all three: loss and gradient of the present weights over rows d_idx [n_m][B], every member on its own rows
static int enqueue_grad(clothhip_handle *h, const FitNet &net, const FitPlan &p, const FitLoss &loss, int32_t n_m, const int32_t *d_idx, int32_t B, double *d_stats,
                        float *d_ratio, float *d_ls) {
    const FitWork w = fit_work(h->fit.own);
    if (int rc = enqueue_forward(h, net.D, p, n_m, d_idx, B, false, w)) return rc;
    if (int rc = enqueue_loss(h, net, p, loss, n_m, d_idx, B, d_stats, d_ratio, d_ls, w)) return rc;
    return enqueue_backward(h, net.D, p, n_m, d_idx, B, w);
}

// loss and gradient of `members` over idx [n_m][B], nothing updated; the call is valid
static int run_grad(clothhip_handle *h, const FitNet &net, const FitLoss &loss, const int32_t *members, int32_t n_m, const int32_t *idx, int32_t B, const FitOut &out) {
    auto &f = h->fit;
    const FitPlan p = fit_plan(net.D, B);
    const size_t n_loss = (size_t)n_m * loss.stats;
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = fit_reserve(h, p, n_m)) return rc;
    if (loss.kind == FitLoss::PPO_SIGMA) if (int rc = f.d_grad_ls.reserve((size_t)n_m * MLP_OUT * 4)) return rc;
    if (int rc = f.d_idx.reserve((size_t)n_m * B * 4)) return rc;
    if (int rc = f.d_loss.reserve(n_loss * 8)) return rc;
    if (out.ratio) if (int rc = f.d_ratio.reserve((size_t)n_m * B * 4)) return rc;
    if (loss.kind == FitLoss::PPO) {      // the members' constants, one row for the shared network
        if (int rc = f.d_ppo_q.reserve((size_t)n_m * 32)) return rc;
        HIPCHECK(hipMemcpyAsync(f.d_ppo_q, loss.q, (size_t)n_m * 32, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHECK(hipMemcpyAsync(f.d_members, members, (size_t)n_m * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_idx, idx, (size_t)n_m * B * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    if (int rc = enqueue_grad(h, net, p, loss, n_m, f.d_idx, B, f.d_loss, out.ratio ? (float *)f.d_ratio : nullptr, nullptr)) return rc;
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    if (out.grad) HIPCHECK(hipMemcpyAsync(out.grad, f.own.d_grad, (size_t)n_m * p.grad * 4, hipMemcpyDeviceToHost, h->stream));
    if (out.loss) HIPCHECK(hipMemcpyAsync(out.loss, f.d_loss, n_loss * 8, hipMemcpyDeviceToHost, h->stream));
    if (out.ratio) HIPCHECK(hipMemcpyAsync(out.ratio, f.d_ratio, (size_t)n_m * B * 4, hipMemcpyDeviceToHost, h->stream));
    if (out.grad_ls) HIPCHECK(hipMemcpyAsync(out.grad_ls, f.d_grad_ls, (size_t)n_m * MLP_OUT * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_policy_fit_grad(clothhip_handle *h, const int32_t *idx, int32_t B, float *grad_out, double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, B, B)) return rc;
    return run_grad(h, policy_net(h), squared_error(), SHARED_ROW, 1, idx, B, {loss_out, grad_out});
}

extern "C" int clothhip_policy_fit_grad_members(clothhip_handle *h, const int32_t *members, int32_t n_m, const int32_t *idx, int32_t B, float *grad_out,
                                                double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, true)) return rc;
    if (int rc = check_fit_members(h, members, n_m)) return rc;
    if (int rc = check_fit_rows(h, n_m, idx, (int64_t)n_m * B, B)) return rc;
    return run_grad(h, policy_net(h), squared_error(), members, n_m, idx, B, {loss_out, grad_out});
}

// The loss alone of the shared network over any number of rows: chunks of at most FIT_MAX_BATCH through the forward pass above, each
// chunk's weighted sum of squares in k_fit_loss's order (k_fit_sqsum), the chunk sums added in ascending order in double on the host, divided
// once by 4 n.
extern "C" int clothhip_policy_fit_loss(clothhip_handle *h, const int32_t *idx, int64_t n, double *loss) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (n < 1 || n > INT32_MAX) return fail(CLOTHHIP_EINVAL, "n = %lld outside [1, %d]", (long long)n, INT32_MAX);
    const int32_t Bmax = (int32_t)std::min<int64_t>(n, FIT_MAX_BATCH);
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, n, Bmax)) return rc;
    if (!loss) return fail(CLOTHHIP_EINVAL, "NULL argument");
    auto &f = h->fit;
    const FitNet net = policy_net(h);
    const int L = h->pol.mlp.n_layers;
    const int64_t n_chunks = (n + FIT_MAX_BATCH - 1) / FIT_MAX_BATCH;
    std::vector<double> sums;
    try { sums.resize((size_t)n_chunks); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld chunks)", (long long)n_chunks); }
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = fit_reserve(h, fit_plan(net.D, Bmax), 1)) return rc;
    if (int rc = f.d_idx.reserve((size_t)n * 4)) return rc;
    if (int rc = f.d_loss.reserve((size_t)n_chunks * 8)) return rc;
    HIPCHECK(hipMemcpyAsync(f.d_members, SHARED_ROW, 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_idx, idx, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    for (int64_t c = 0; c < n_chunks; c++) {
        const int32_t B = (int32_t)std::min<int64_t>(FIT_MAX_BATCH, n - c * FIT_MAX_BATCH);
        const FitPlan p = fit_plan(net.D, B);
        const int32_t *d_idx = f.d_idx + (size_t)c * FIT_MAX_BATCH;
        if (int rc = enqueue_forward(h, net.D, p, 1, d_idx, B, false, fit_work(f.own))) return rc;
        launch_fit_sqsum(h->stream, f.own.d_act + p.h_off[L - 1], h->dataset.lab(), h->dataset.w(), d_idx, B, f.d_loss + c);
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    HIPCHECK(hipMemcpyAsync(sums.data(), f.d_loss, (size_t)n_chunks * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    double s = sums[0];
    for (int64_t c = 1; c < n_chunks; c++) s = s + sums[c];
    *loss = s / (double)(4 * n);
    return 0;
}

// The forward alone on n stored rows, the same rows for every member: chunks through enqueue_forward, each chunk's y copied out to
// d_pred [n_m][n][net.out()] (k_fit_copy_y), where it stays: enqueued between the timing events, not synchronised. The call is valid.
// dst (NULL: d_pred; else n_m == 1): the table that gets y in the place of d_pred, [n][net.out()] -- a dataset column that is written where it lies.
int enqueue_predict(clothhip_handle *h, const FitNet &net, const int32_t *members, int32_t n_m, const int32_t *idx, int64_t n, float *dst) {
    auto &f = h->fit;
    const int L = net.D.n_layers, W = net.out();
    const int32_t Bmax = (int32_t)std::min<int64_t>(n, std::min<int64_t>(FIT_MAX_BATCH, CLOTHHIP_FIT_MAX_MEMBER_ROWS / n_m));
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = fit_reserve(h, fit_plan(net.D, Bmax), n_m)) return rc;
    if (int rc = f.d_idx.reserve((size_t)n * 4)) return rc;
    if (!dst) {
        if (int rc = f.d_pred.reserve((size_t)n_m * n * W * 4)) return rc;
        dst = f.d_pred;
    }
    HIPCHECK(hipMemcpyAsync(f.d_members, members, (size_t)n_m * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_idx, idx, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    for (int64_t r0 = 0; r0 < n; r0 += Bmax) {
        const int32_t B = (int32_t)std::min<int64_t>(Bmax, n - r0);
        const FitPlan p = fit_plan(net.D, B);
        if (int rc = enqueue_forward(h, net.D, p, n_m, f.d_idx + (size_t)r0, B, true, fit_work(f.own))) return rc;
        const int32_t blocks = (W * B + 255) / 256;
        launch_fit_copy_y(h->stream, n_m, f.own.d_act + p.h_off[L - 1], W * B, dst + (size_t)r0 * W, (int64_t)p.act, (int64_t)n * W, blocks);
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    return 0;
}
// ... and one download
static int run_predict(clothhip_handle *h, const FitNet &net, const int32_t *members, int32_t n_m, const int32_t *idx, int64_t n, float *y_out) {
    if (int rc = enqueue_predict(h, net, members, n_m, idx, n, nullptr)) return rc;
    HIPCHECK(hipMemcpyAsync(y_out, h->fit.d_pred, (size_t)n_m * n * net.out() * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_policy_fit_predict(clothhip_handle *h, const int32_t *idx, int64_t n, float *y_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (n < 1 || n > INT32_MAX) return fail(CLOTHHIP_EINVAL, "n = %lld outside [1, %d]", (long long)n, INT32_MAX);
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, n, (int32_t)std::min<int64_t>(n, FIT_MAX_BATCH))) return rc;
    if (!y_out) return fail(CLOTHHIP_EINVAL, "NULL argument");
    return run_predict(h, policy_net(h), SHARED_ROW, 1, idx, n, y_out);
}

extern "C" int clothhip_policy_fit_predict_members(clothhip_handle *h, const int32_t *members, int32_t n_m, const int32_t *idx, int64_t n, float *y_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, true)) return rc;
    if (n < 1 || n > INT32_MAX) return fail(CLOTHHIP_EINVAL, "n = %lld outside [1, %d]", (long long)n, INT32_MAX);
    if (int rc = check_fit_members(h, members, n_m)) return rc;
    if (n_m > CLOTHHIP_FIT_MAX_MEMBER_ROWS) return fail(CLOTHHIP_EINVAL, "n_m = %d members in one call, at most %d", n_m, CLOTHHIP_FIT_MAX_MEMBER_ROWS);
    if (int rc = check_fit_rows(h, 1, idx, n, 1)) return rc;
    if (!y_out) return fail(CLOTHHIP_EINVAL, "NULL argument");
    return run_predict(h, policy_net(h), members, n_m, idx, n, y_out);
}

// ---- the optimizer ----------------------------------------------------------------------------------------------------------------------
// the per-row optimizer state exists from the first step after a new network: every row fresh. false: out of host memory, and forgotten
static bool ensure_row_state(OptState &o, size_t rows) {
    if (o.t.size() == rows && o.zero.size() == rows) return true;
    try { o.t.assign(rows, 0); o.zero.assign(rows, 1); } catch (const std::bad_alloc &) { o.forget(); return false; }
    return true;
}

// The step constants q [FIT_HYPER] of ONE optimizer step under p, the t1-th of its row (1-based): made in double, then rounded to float
static void step_constants(float *q, const ClothFitParams &p, bool adam, int64_t t1) {
    if (adam) {
        const double b1 = (double)p.beta1, b2 = (double)p.beta2, td = (double)t1;
        const double a_t = (double)p.lr * std::sqrt(1.0 - std::pow(b2, td)) / (1.0 - std::pow(b1, td));
        q[0] = (float)a_t; q[1] = p.beta1; q[2] = (float)(1.0 - b1); q[3] = p.beta2; q[4] = (float)(1.0 - b2); q[5] = p.eps;
    } else {
        q[0] = p.lr; q[1] = p.momentum;
    }
}
// The optimizer's bookkeeping of a call (OptTarget, OptPlan: fit_trainer.hpp), the ONE place that keeps a row's step count and its
// read-as-zeros flag right across calls of different losses on one OptState. A net's rows as a target:
OptTarget net_target(const FitNet &net, const int32_t *members, int32_t n_m, const Buffer<float> &grad, const ClothFitParams *p) {
    return {net.theta, &net.opt, net.rows(), net.pop_rows ? (size_t)net.pop_rows * net.D.stride : net.n_params, (int64_t)net.D.stride, (int64_t)net.n_params, members, n_m, &grad, p, 0};
}
// 1. host only, nothing of the handle changes (but that fresh per-row state comes to exist): the step constants of every (target, step,
// member), in double on the host, then rounded to float
int opt_prepare(OptPlan &o, int32_t n_steps) {
    o.n_steps = n_steps;
    size_t n_hyper = 0;
    for (int k = 0; k < o.n; k++) { o.t[k].hyper_at = n_hyper; n_hyper += (size_t)n_steps * o.t[k].n_m * FIT_HYPER; }
    try { o.hyper.assign(n_hyper, 0.0f); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%zu step constants)", n_hyper); }
    for (int k = 0; k < o.n; k++) {
        const OptTarget &t = o.t[k];
        if (!ensure_row_state(*t.opt, t.rows)) return fail(CLOTHHIP_ENOMEM, "out of host memory (%zu rows)", t.rows);
        for (int s = 0; s < n_steps; s++)
            for (int32_t j = 0; j < t.n_m; j++)
                step_constants(o.hyper.data() + t.hyper_at + ((size_t)s * t.n_m + j) * FIT_HYPER, t.p[j], t.p[0].optimizer == (float)CLOTHHIP_FIT_ADAM, t.opt->t[t.members[j]] + s + 1);
    }
    return 0;
}
// 2. the table of constants and the moments of each target's whole table. A table of another network's size holds no row's state (every
// row is flagged read-as-zeros by OptState::forget when the network changes), so growing it loses nothing
int opt_reserve(clothhip_handle *h, const OptPlan &o) {
    if (o.n) if (int rc = h->fit.d_hyper.reserve(o.hyper.size() * 4)) return rc;
    for (int k = 0; k < o.n; k++) {
        if (int rc = o.t[k].opt->m.reserve(o.t[k].moments * 4)) return rc;
        if (int rc = o.t[k].opt->v.reserve(o.t[k].moments * 4)) return rc;
    }
    return 0;
}
// 3. from here on the call goes through (but for a failure of the runtime itself)
int opt_commit(clothhip_handle *h, OptPlan &o) {
    for (int k = 0; k < o.n; k++) {
        const OptTarget &t = o.t[k];
        for (int32_t j = 0; j < t.n_m; j++) {
            const int32_t g = t.members[j];
            if (t.opt->zero[g]) {
                HIPCHECK(hipMemsetAsync(t.opt->m + (size_t)g * (size_t)t.stride, 0, (size_t)t.n * 4, h->stream));
                HIPCHECK(hipMemsetAsync(t.opt->v + (size_t)g * (size_t)t.stride, 0, (size_t)t.n * 4, h->stream));
                t.opt->zero[g] = 0;
            }
            t.opt->t[g] += o.n_steps;
        }
    }
    if (o.n) HIPCHECK(hipMemcpyAsync(h->fit.d_hyper, o.hyper.data(), o.hyper.size() * 4, hipMemcpyHostToDevice, h->stream));
    return 0;
}
// 4. step s of target k, one launch: its rows h->fit.d_members [n_m] of theta with the moments of opt, row j's gradient at grad + j * n
// and its constants at its place in d_hyper + j * FIT_HYPER
int enqueue_optimizer(clothhip_handle *h, const OptPlan &plan, int k, int s) {
    const OptTarget &t = plan.t[k];
    FitOptArgs o = {};
    o.theta = t.theta; o.m = t.opt->m; o.v = t.opt->v; o.g = *t.grad; o.members = h->fit.d_members;
    o.hyper = h->fit.d_hyper + t.hyper_at + (size_t)s * t.n_m * FIT_HYPER;
    o.stride = t.stride; o.n = t.n; o.blocks = (int32_t)((t.n + 255) / 256);
    const dim3 ogrid((unsigned)o.blocks * (unsigned)t.n_m);
    if (t.p[0].optimizer == (float)CLOTHHIP_FIT_ADAM) hipLaunchKernelGGL(k_fit_adam, ogrid, dim3(256), 0, h->stream, o);
    else hipLaunchKernelGGL(k_fit_sgd, ogrid, dim3(256), 0, h->stream, o);
    HIPCHECK(hipGetLastError());
    return 0;
}

// n_steps optimizer steps of `members` with the optimizers p [n_m] over idx [n_steps][n_m][B]; the call is valid and n_steps >= 1. The
// optimizer walks one target, the net's rows, and under PPO_SIGMA (n_m == 1) a second one: the log-sigma head, a table of one row of
// four elements at offset 0 with its own state h->fit.opt_sigma and its own step constants, made from p[0].
static int run_fit(clothhip_handle *h, const FitNet &net, const FitLoss &loss, const ClothFitParams *p, const int32_t *members, int32_t n_m, const int32_t *idx,
                   int32_t n_steps, int32_t B, const FitOut &out) {
    auto &f = h->fit;
    const FitPlan pl = fit_plan(net.D, B);
    const size_t n_sm = (size_t)n_steps * n_m;
    const bool head = loss.kind == FitLoss::PPO_SIGMA;
    OptPlan opt;
    opt.add(net_target(net, members, n_m, f.own.d_grad, p));
    if (head) opt.add({h->pol.d_log_sigma, &f.opt_sigma, 1, MLP_OUT, 0, MLP_OUT, SHARED_ROW, 1, &f.d_grad_ls, p, 0});
    if (int rc = opt_prepare(opt, n_steps)) return rc;
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = fit_reserve(h, pl, n_m)) return rc;
    if (int rc = f.d_idx.reserve(n_sm * B * 4)) return rc;
    if (int rc = f.d_loss.reserve(n_sm * loss.stats * 8)) return rc;
    if (loss.kind == FitLoss::PPO) if (int rc = f.d_ppo_q.reserve((size_t)n_m * 32)) return rc;
    if (head) {
        if (int rc = f.d_grad_ls.reserve(MLP_OUT * 4)) return rc;
        if (int rc = f.d_ls_hist.reserve((size_t)n_steps * MLP_OUT * 4)) return rc;
    }
    if (int rc = opt_reserve(h, opt)) return rc;
    if (int rc = opt_commit(h, opt)) return rc;
    HIPCHECK(hipMemcpyAsync(f.d_members, members, (size_t)n_m * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_idx, idx, n_sm * B * 4, hipMemcpyHostToDevice, h->stream));
    if (loss.kind == FitLoss::PPO) HIPCHECK(hipMemcpyAsync(f.d_ppo_q, loss.q, (size_t)n_m * 32, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    for (int s = 0; s < n_steps; s++) {
        if (int rc = enqueue_grad(h, net, pl, loss, n_m, f.d_idx + (size_t)s * n_m * B, B, f.d_loss + (size_t)s * n_m * loss.stats, nullptr,
                                  head ? f.d_ls_hist + (size_t)s * MLP_OUT : nullptr)) return rc;
        for (int k = 0; k < opt.n; k++)      // (the head names its row 0 by the call's own member table: n_m == 1, members = {0})
            if (int rc = enqueue_optimizer(h, opt, k, s)) return rc;
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    if (out.loss) HIPCHECK(hipMemcpyAsync(out.loss, f.d_loss, n_sm * loss.stats * 8, hipMemcpyDeviceToHost, h->stream));
    if (head && out.ls) HIPCHECK(hipMemcpyAsync(out.ls, f.d_ls_hist, (size_t)n_steps * MLP_OUT * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));      // (the host tables are never retained)
    return 0;
}

extern "C" int clothhip_policy_fit(clothhip_handle *h, const ClothFitParams *p, const int32_t *idx, int32_t n_steps, int32_t B, double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!p) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, (int64_t)n_steps * B, B)) return rc;
    if (int rc = check_fit_params(p, -1)) return rc;
    if (n_steps == 0) return 0;
    return run_fit(h, policy_net(h), squared_error(), p, SHARED_ROW, 1, idx, n_steps, B, {loss_out});
}

extern "C" int clothhip_policy_fit_members(clothhip_handle *h, const ClothFitParams *p, const int32_t *members, int32_t n_m, const int32_t *idx,
                                           int32_t n_steps, int32_t B, double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, true)) return rc;
    if (!p) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_fit_members(h, members, n_m)) return rc;
    if (int rc = check_fit_rows(h, n_m, idx, (int64_t)n_steps * n_m * B, B)) return rc;
    if (int rc = check_fit_params_members(p, n_m)) return rc;
    if (n_steps == 0) return 0;
    return run_fit(h, policy_net(h), squared_error(), p, members, n_m, idx, n_steps, B, {loss_out});
}

extern "C" int clothhip_policy_fit_reset(clothhip_handle *h) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    h->fit.opt_policy.forget();
    h->fit.opt_sigma.forget();      // the head is trained with the policy
    return 0;
}

extern "C" int clothhip_policy_fit_reset_members(clothhip_handle *h, const int32_t *members, int32_t n_m) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_population first");
    if (!h->pol.pop_rows) return fail(CLOTHHIP_ESTATE, "this handle holds ONE shared network, not a population: use clothhip_policy_fit_reset");
    if (!members) { h->fit.opt_policy.forget(); return 0; }      // all rows
    if (int rc = check_fit_members(h, members, n_m)) return rc;
    if (h->fit.opt_policy.t.empty()) return 0;               // every row is fresh already
    for (int32_t j = 0; j < n_m; j++) { h->fit.opt_policy.t[members[j]] = 0; h->fit.opt_policy.zero[members[j]] = 1; }
    return 0;
}

// ---- PPO: the old means and the clipped surrogate as one more loss mode of the trainer above (clothhip.h: PPO ON THE DEVICE) --------------
static_assert(FIT_PPO_STATS == CLOTHHIP_PPO_STATS, "the statistics of the header and of the kernel");
static_assert(sizeof(ClothPpoParams) == 16, "ClothPpoParams is two doubles");

// the constants of member j of a PPO call (j < 0: of the shared network, named without an index) -> row [4], the kernel's constants
static int check_ppo_consts(const ClothPpoParams *q, int32_t j, double *row) {
    char who[24] = "";
    if (j >= 0) snprintf(who, sizeof(who), "q[%d]: ", j);
    if (!std::isfinite(q->sigma) || q->sigma <= 0.0) return fail(CLOTHHIP_EINVAL, "%ssigma = %g: the policy's standard deviation is finite and > 0", who, q->sigma);
    if (!std::isfinite(q->clip) || q->clip < 0.0 || q->clip >= 1.0) return fail(CLOTHHIP_EINVAL, "%sclip = %g: the clip range lies in [0, 1)", who, q->clip);
    const double s2 = q->sigma * q->sigma;
    row[0] = 1.0 / s2;
    row[1] = 0.5 * row[0];
    row[2] = 1.0 - q->clip;
    row[3] = 1.0 + q->clip;
    if (!std::isfinite(row[0])) return fail(CLOTHHIP_EINVAL, "%ssigma = %g: 1 / sigma^2 is not a finite double", who, q->sigma);
    return 0;
}
// every row of the minibatches idx [n_steps][n_m][B] (n_idx entries) has its old mean and, log_sigma: its old log sigma. members
// NULL: the shared network's call (n_m == 1), else the refusal names the member whose row it is
static int check_old_set(const clothhip_handle *h, const int32_t *members, int32_t n_m, const int32_t *idx, int64_t n_idx, int32_t B, bool log_sigma) {
    for (int64_t i = 0; i < n_idx; i++) {
        if (!h->dataset.h_old_set[(size_t)idx[i]]) {
            char who[40] = "";
            if (members) snprintf(who, sizeof(who), " of member %lld", (long long)members[(i / B) % n_m]);
            return fail(CLOTHHIP_ESTATE, "idx[%lld] = row %d%s has no old mean: call clothhip_fit_data_snapshot_policy%s or clothhip_fit_data_set_old_means on it first",
                        (long long)i, idx[i], who, members ? "_members" : "");
        }
        if (log_sigma && !h->dataset.h_old_ls_set[(size_t)idx[i]])
            return fail(CLOTHHIP_ESTATE, "idx[%lld] = row %d has no old log sigma: call clothhip_fit_data_snapshot_policy (with the head on the handle) or clothhip_fit_data_set_old_log_sigma on it first",
                        (long long)i, idx[i]);
    }
    return 0;
}
// the constants q [n_m] of a PPO call and the rows of its minibatches, after everything clothhip_policy_fit / _members refuses:
// -> tab [n_m][4], the table k_fit_loss_ppo reads. members NULL: the shared network's call, a table of one row
static int check_ppo(const clothhip_handle *h, const ClothPpoParams *q, const int32_t *members, int32_t n_m, const int32_t *idx, int64_t n_idx, int32_t B,
                     std::vector<double> *tab) {
    try { tab->resize((size_t)n_m * 4); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%d members)", n_m); }
    for (int32_t j = 0; j < n_m; j++)
        if (int rc = check_ppo_consts(q + j, members ? j : -1, tab->data() + (size_t)j * 4)) return rc;
    return check_old_set(h, members, n_m, idx, n_idx, B, false);
}

extern "C" int clothhip_policy_fit_ppo_grad(clothhip_handle *h, const ClothPpoParams *q, const int32_t *idx, int32_t B, float *grad_out, double *stats_out,
                                            float *ratio_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, B, B)) return rc;
    std::vector<double> tab;
    if (int rc = check_ppo(h, q, nullptr, 1, idx, B, B, &tab)) return rc;
    return run_grad(h, policy_net(h), ppo_loss(tab.data()), SHARED_ROW, 1, idx, B, {stats_out, grad_out, ratio_out});
}

extern "C" int clothhip_policy_fit_ppo(clothhip_handle *h, const ClothFitParams *p, const ClothPpoParams *q, const int32_t *idx, int32_t n_steps, int32_t B,
                                       double *stats_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!p || !q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, (int64_t)n_steps * B, B)) return rc;
    if (int rc = check_fit_params(p, -1)) return rc;
    std::vector<double> tab;
    if (int rc = check_ppo(h, q, nullptr, 1, idx, (int64_t)n_steps * B, B, &tab)) return rc;
    if (n_steps == 0) return 0;
    return run_fit(h, policy_net(h), ppo_loss(tab.data()), p, SHARED_ROW, 1, idx, n_steps, B, {stats_out});
}

// ---- PPO for a population (clothhip.h: PPO FOR A POPULATION): the two entries above as grouped calls (the snapshot by member: api_fit_rollout.hip) ----
extern "C" int clothhip_policy_fit_ppo_grad_members(clothhip_handle *h, const ClothPpoParams *q, const int32_t *members, int32_t n_m, const int32_t *idx, int32_t B,
                                                    float *grad_out, double *stats_out, float *ratio_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, true)) return rc;
    if (!q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_fit_members(h, members, n_m)) return rc;
    if (int rc = check_fit_rows(h, n_m, idx, (int64_t)n_m * B, B)) return rc;
    std::vector<double> tab;
    if (int rc = check_ppo(h, q, members, n_m, idx, (int64_t)n_m * B, B, &tab)) return rc;
    return run_grad(h, policy_net(h), ppo_loss(tab.data()), members, n_m, idx, B, {stats_out, grad_out, ratio_out});
}

extern "C" int clothhip_policy_fit_ppo_members(clothhip_handle *h, const ClothFitParams *p, const ClothPpoParams *q, const int32_t *members, int32_t n_m,
                                               const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, true)) return rc;
    if (!p || !q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_fit_members(h, members, n_m)) return rc;
    if (int rc = check_fit_rows(h, n_m, idx, (int64_t)n_steps * n_m * B, B)) return rc;
    if (int rc = check_fit_params_members(p, n_m)) return rc;
    std::vector<double> tab;
    if (int rc = check_ppo(h, q, members, n_m, idx, (int64_t)n_steps * n_m * B, B, &tab)) return rc;
    if (n_steps == 0) return 0;
    return run_fit(h, policy_net(h), ppo_loss(tab.data()), p, members, n_m, idx, n_steps, B, {stats_out});
}

// ---- PPO with a learned sigma: one more loss mode, and the head as one more table of the optimizer (clothhip.h: PPO WITH A LEARNED SIGMA) ----
static_assert(FIT_PPO_SIGMA_STATS == CLOTHHIP_PPO_SIGMA_STATS, "the statistics of the header and of the kernel");
static_assert(sizeof(ClothPpoSigmaParams) == 16, "ClothPpoSigmaParams is two doubles");

// the constants of such a call and the rows of its minibatches, after everything clothhip_policy_fit refuses: -> the loss
static int check_ppo_sigma(const clothhip_handle *h, const ClothPpoSigmaParams *q, const int32_t *idx, int64_t n_idx, int32_t B, FitLoss *out) {
    if (!std::isfinite(q->clip) || q->clip < 0.0 || q->clip >= 1.0) return fail(CLOTHHIP_EINVAL, "clip = %g: the clip range lies in [0, 1)", q->clip);
    if (!std::isfinite(q->ent_coef) || q->ent_coef < 0.0) return fail(CLOTHHIP_EINVAL, "ent_coef = %g: the entropy coefficient is finite and >= 0", q->ent_coef);
    *out = ppo_sigma_loss(1.0 - q->clip, 1.0 + q->clip, q->ent_coef);
    return check_old_set(h, nullptr, 1, idx, n_idx, B, true);
}
static int check_head(const clothhip_handle *h) {
    if (!h->pol.has_log_sigma) return fail(CLOTHHIP_ESTATE, "no log-sigma head on this handle: call clothhip_set_policy_log_sigma first");
    return 0;
}

extern "C" int clothhip_policy_fit_ppo_sigma_grad(clothhip_handle *h, const ClothPpoSigmaParams *q, const int32_t *idx, int32_t B, float *grad_out, float *grad_ls_out,
                                                  double *stats_out, float *ratio_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_head(h)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, B, B)) return rc;
    FitLoss loss;
    if (int rc = check_ppo_sigma(h, q, idx, B, B, &loss)) return rc;
    return run_grad(h, policy_net(h), loss, SHARED_ROW, 1, idx, B, {stats_out, grad_out, ratio_out, grad_ls_out});
}

extern "C" int clothhip_policy_fit_ppo_sigma(clothhip_handle *h, const ClothFitParams *p, const ClothPpoSigmaParams *q, const int32_t *idx, int32_t n_steps, int32_t B,
                                             double *stats_out, float *log_sigma_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!p || !q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_head(h)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, (int64_t)n_steps * B, B)) return rc;
    if (int rc = check_fit_params(p, -1)) return rc;
    FitLoss loss;
    if (int rc = check_ppo_sigma(h, q, idx, (int64_t)n_steps * B, B, &loss)) return rc;
    if (n_steps == 0) return 0;
    return run_fit(h, policy_net(h), loss, p, SHARED_ROW, 1, idx, n_steps, B, {stats_out, nullptr, nullptr, nullptr, log_sigma_out});
}

// ---- the critic: the value network as one more one-row table of the trainer above (clothhip.h: FITTING THE CRITIC) ------------------------
extern "C" int clothhip_value_fit_grad(clothhip_handle *h, const int32_t *idx, int32_t B, float *grad_out, double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_value_state(h)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, B, B)) return rc;
    return run_grad(h, value_net(h), squared_error(), SHARED_ROW, 1, idx, B, {loss_out, grad_out});
}

extern "C" int clothhip_value_fit(clothhip_handle *h, const ClothFitParams *p, const int32_t *idx, int32_t n_steps, int32_t B, double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!p) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_value_state(h)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, (int64_t)n_steps * B, B)) return rc;
    if (int rc = check_fit_params(p, -1)) return rc;
    if (n_steps == 0) return 0;
    return run_fit(h, value_net(h), squared_error(), p, SHARED_ROW, 1, idx, n_steps, B, {loss_out});
}

extern "C" int clothhip_value_fit_reset(clothhip_handle *h) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    h->fit.opt_value.forget();
    return 0;
}

extern "C" int clothhip_value_predict(clothhip_handle *h, const int32_t *idx, int64_t n, float *v_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (n < 1 || n > INT32_MAX) return fail(CLOTHHIP_EINVAL, "n = %lld outside [1, %d]", (long long)n, INT32_MAX);
    if (int rc = check_value_state(h)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, n, (int32_t)std::min<int64_t>(n, FIT_MAX_BATCH))) return rc;
    if (!v_out) return fail(CLOTHHIP_EINVAL, "NULL argument");
    return run_predict(h, value_net(h), SHARED_ROW, 1, idx, n, v_out);
}

// ---- DDPG's launches (api_fit_ddpg.hip has the entries and the order; cloth_fit_ddpg.hpp the kernels) ---------------------------------------
static_assert(FIT_TD_STATS + FIT_DPG_STATS == CLOTHHIP_DDPG_STATS && FIT_TD_STATS == CLOTHHIP_Q_STATS && FIT_DPG_STATS == CLOTHHIP_DPG_STATS, "the statistics of the header and of the kernels");
static_assert(FIT_DPG_BC_STATS == CLOTHHIP_DPG_BC_STATS && FIT_TD_STATS + FIT_DPG_BC_STATS == CLOTHHIP_DDPG_BC_STATS, "the statistics of the header and of the BC kernel");
static_assert(FIT_NO_EXPERT == FIT_COL[COL_EXP].fill, "the expert column's fill as the kernels test it");
static_assert(FIT_NEXT_TERMINAL == CLOTHHIP_FIT_NEXT_TERMINAL, "the terminal mark of the header and of the kernel");

int enqueue_concat(clothhip_handle *h, bool label, const float *act, const int32_t *d_rows, int32_t B, float bound) {
    FitConcatArgs c = {};
    c.obs = h->dataset.obs(); c.lab = h->dataset.lab(); c.act = act; c.rows = d_rows; c.X = h->fit.d_qx; c.bound = bound; c.B = B; c.L = 3 * h->P;
    if (label) hipLaunchKernelGGL(k_fit_concat<true>, dim3((unsigned)B), dim3(FIT_DDPG_THREADS), 0, h->stream, c);
    else hipLaunchKernelGGL(k_fit_concat<false>, dim3((unsigned)B), dim3(FIT_DDPG_THREADS), 0, h->stream, c);
    HIPCHECK(hipGetLastError());
    return 0;
}
int enqueue_concat_expert(clothhip_handle *h, const int32_t *d_rows, int32_t B, float bound) {
    FitConcatArgs c = {};
    c.obs = h->dataset.obs(); c.lab = h->dataset.expert(); c.rows = d_rows; c.X = h->fit.d_qxe; c.bound = bound; c.B = B; c.L = 3 * h->P;
    hipLaunchKernelGGL((k_fit_concat<true, true>), dim3((unsigned)B), dim3(FIT_DDPG_THREADS), 0, h->stream, c);
    HIPCHECK(hipGetLastError());
    return 0;
}
int enqueue_polyak(clothhip_handle *h, double tau) {
    const float t = (float)tau, omt = (float)(1.0 - tau);
    const int64_t n[2] = {(int64_t)h->pol.mlp_n_params, (int64_t)h->qnet.n_params};
    float *target[2] = {h->tgt.d_policy, h->tgt.d_q};
    const float *theta[2] = {h->pol.d_mlp, h->qnet.d_mlp};
    for (int k = 0; k < 2; k++) {
        hipLaunchKernelGGL(k_fit_polyak, dim3((unsigned)((n[k] + FIT_DDPG_THREADS - 1) / FIT_DDPG_THREADS)), dim3(FIT_DDPG_THREADS), 0, h->stream, target[k], theta[k], n[k], t, omt);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}
// dL/da [B][4] into h->fit.d_da from the dZ of the critic's last layer (in w.dz): the input gradients of the NN product with the mask
// epilogue down to layer 0, then layer 0's for the four action columns alone. No weight gradient is formed.
int enqueue_action_grad(clothhip_handle *h, const MlpDesc &D, const FitPlan &p, int32_t B, const FitWork &w) {
    for (int l = D.n_layers - 1; l > 0; l--) if (int rc = enqueue_input_grad(h, D, p, l, 1, B, w)) return rc;
    const int n_in = D.widths[0], n_out = D.widths[1];
    FitGemmArgs b = {};
    b.members = h->fit.d_members; b.stride = D.stride;
    b.A = w.dz; b.lda = n_out;
    b.B = D.params + p.w_off[0] + (n_in - MLP_OUT); b.ldb = n_in; b.b_weights = 1;      // W_0's action columns: the last four of a row of 3P + 4
    b.C = h->fit.d_da; b.ldc = MLP_OUT;
    b.M = B; b.N = MLP_OUT; b.K = n_out; b.k_chunk = n_out;
    launch_gemm<true, false, FIT_EPI_NONE, false>(h->stream, b, 1);
    HIPCHECK(hipGetLastError());
    return 0;
}
// cloth_policy_fit.hpp's k_fit_fill_ls: the handle's present log sigma into n4 / 4 rows of four at dst
int enqueue_fill_ls(clothhip_handle *h, float *dst, int64_t n4) {
    hipLaunchKernelGGL(k_fit_fill_ls, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, h->stream, dst, (const float *)h->pol.d_log_sigma, n4);
    HIPCHECK(hipGetLastError());
    return 0;
}
