// api_fit_rollout.hip -- the entries that fill dataset columns from a forward pass of the handle's present networks, through the launches of api_fit.hip (fit_trainer.hpp): the snapshot of the old means (and, with a log-sigma head, of the old log sigma; for a population by the member that acted), and advantages and value targets from the critic's values. The one includer of cloth_fit_gae.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <utility>
#include <vector>

#include "cloth_fit_gae.hpp"
#include "fit_trainer.hpp"

static_assert(GAE_NEXT_NONE == CLOTHHIP_FIT_NEXT_NONE && CLOTHHIP_FIT_NEXT_TERMINAL < 0 && CLOTHHIP_FIT_NEXT_NONE < 0, "the leaf mark of the header and of the kernels");
static_assert(sizeof(ClothGaeParams) == 24, "ClothGaeParams is two doubles, a float and an int32");

// ---- PPO: the old means (clothhip.h: PPO ON THE DEVICE) ------------------------------------------------------------------------------------
extern "C" int clothhip_fit_data_snapshot_policy(clothhip_handle *h, int64_t first, int64_t n) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_range(h, first, n)) return rc;
    if (n == 0) return 0;
    std::vector<int32_t> idx;
    try { idx.resize((size_t)n); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)n); }
    for (int64_t i = 0; i < n; i++) idx[(size_t)i] = (int32_t)(first + i);
    // the launches of clothhip_policy_fit_predict; each chunk's y goes to its rows of the column, which are consecutive
    if (int rc = enqueue_predict(h, policy_net(h), SHARED_ROW, 1, idx.data(), n, h->dataset.old() + (size_t)first * 4)) return rc;
    // with a head: the present log sigma into the same rows of its column, on the device (the predict moved ev1 behind itself; so does this)
    if (h->pol.has_log_sigma) {
        if (int rc = enqueue_fill_ls(h, h->dataset.old_ls() + (size_t)first * MLP_OUT, n * MLP_OUT)) return rc;
        HIPCHECK(hipEventRecord(h->ev1, h->stream));
    }
    HIPCHECK(hipStreamSynchronize(h->stream));      // (idx, a host table the upload read, goes out of scope)
    h->dataset.mark_old_set(first, n);
    if (h->pol.has_log_sigma) h->dataset.mark_old_ls_set(first, n);
    return 0;
}

// ---- PPO for a population (clothhip.h: PPO FOR A POPULATION): the snapshot by member ---------------------------------------------------------
// The forward of n_m members on THEIR OWN rows, scattered to the old-mean column. The rows named are grouped by member; member lists
// longer than CLOTHHIP_FIT_MAX_BATCH are cut into segments, and the k-th segments of all members that have one are launched together,
// longest first, as many as CLOTHHIP_FIT_MAX_MEMBER_ROWS holds at the longest one's length B. A shorter segment is padded to B with its
// own first row (a valid row of the same member: the layer-0 gather stays in range), which k_fit_scatter_y does not store.
struct SnapChunk { size_t m0, idx0; int32_t n_m, B; };      // offsets into the call's member / length tables and its index table
struct SnapPlan {
    std::vector<int32_t> mem, len, idx;      // per chunk member: the population row and its real positions; the index tables [n_m][B], chunk after chunk
    std::vector<SnapChunk> chunks;           // none: no row names a member
};
// the plan of rows [first, first + n) under member_of_row (every entry in [-1, pop_rows))
static int plan_snapshot(int64_t pop_rows, int64_t first, int64_t n, const int32_t *member_of_row, SnapPlan *out) {
    std::vector<int32_t> &mem = out->mem, &len = out->len, &idx = out->idx;
    try {
        // the rows of every member, ascending, as one table sorted by (member, row): start[g] .. start[g + 1]
        std::vector<int64_t> start((size_t)pop_rows + 1, 0);
        for (int64_t i = 0; i < n; i++) if (member_of_row[i] >= 0) start[(size_t)member_of_row[i] + 1]++;
        for (size_t g = 0; g < (size_t)pop_rows; g++) start[g + 1] += start[g];
        const int64_t named = start[(size_t)pop_rows];
        if (named == 0) return 0;
        std::vector<int32_t> by_member((size_t)named);
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int64_t i = 0; i < n; i++) if (member_of_row[i] >= 0) by_member[(size_t)at[(size_t)member_of_row[i]]++] = (int32_t)(first + i);
        for (int64_t k = 0;; k++) {          // the k-th segments
            std::vector<std::pair<int32_t, int32_t>> seg;      // (length, member), longest first
            for (int64_t g = 0; g < pop_rows; g++) {
                const int64_t rest = start[(size_t)g + 1] - start[(size_t)g] - k * CLOTHHIP_FIT_MAX_BATCH;
                if (rest > 0) seg.push_back({(int32_t)std::min<int64_t>(rest, CLOTHHIP_FIT_MAX_BATCH), (int32_t)g});
            }
            if (seg.empty()) break;
            std::stable_sort(seg.begin(), seg.end(), [](const std::pair<int32_t, int32_t> &a, const std::pair<int32_t, int32_t> &b) { return a.first > b.first; });
            for (size_t s0 = 0; s0 < seg.size();) {
                const int32_t B = seg[s0].first;
                const size_t n_m = std::min<size_t>(seg.size() - s0, (size_t)(CLOTHHIP_FIT_MAX_MEMBER_ROWS / B));
                out->chunks.push_back({mem.size(), idx.size(), (int32_t)n_m, B});
                for (size_t j = s0; j < s0 + n_m; j++) {
                    const int32_t *rows = by_member.data() + start[(size_t)seg[j].second] + k * CLOTHHIP_FIT_MAX_BATCH;
                    mem.push_back(seg[j].second); len.push_back(seg[j].first);
                    idx.insert(idx.end(), rows, rows + seg[j].first);
                    idx.insert(idx.end(), (size_t)(B - seg[j].first), rows[0]);
                }
                s0 += n_m;
            }
        }
    } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)n); }
    return 0;
}

extern "C" int clothhip_fit_data_snapshot_policy_members(clothhip_handle *h, int64_t first, int64_t n, const int32_t *member_of_row) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, true)) return rc;
    if (int rc = check_range(h, first, n)) return rc;
    if (n == 0) return 0;
    if (!member_of_row) return fail(CLOTHHIP_EINVAL, "member_of_row is NULL");
    for (int64_t i = 0; i < n; i++)
        if (member_of_row[i] < -1 || member_of_row[i] >= h->pol.pop_rows)
            return fail(CLOTHHIP_EINVAL, "member_of_row[%lld] = %d outside [-1, %lld)", (long long)i, member_of_row[i], (long long)h->pol.pop_rows);
    auto &f = h->fit;
    const FitNet net = policy_net(h);
    const int L = net.D.n_layers;
    SnapPlan s;
    if (int rc = plan_snapshot(h->pol.pop_rows, first, n, member_of_row, &s)) return rc;
    if (s.chunks.empty()) return 0;
    HIPCHECK(hipSetDevice(h->device));
    // every chunk's scratch before the first launch: a buffer that grows is freed first
    for (const SnapChunk &c : s.chunks) if (int rc = fit_reserve(h, fit_plan(net.D, c.B), c.n_m)) return rc;
    if (int rc = f.d_len.reserve(s.len.size() * 4)) return rc;
    if (int rc = f.d_idx.reserve(s.idx.size() * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(f.d_len, s.len.data(), s.len.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_idx, s.idx.data(), s.idx.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    const FitWork w = fit_work(f.own);
    for (const SnapChunk &c : s.chunks) {
        const FitPlan p = fit_plan(net.D, c.B);
        // (the launches read the chunk's members at the head of d_members: stream order keeps the chunks apart)
        HIPCHECK(hipMemcpyAsync(f.d_members, s.mem.data() + c.m0, (size_t)c.n_m * 4, hipMemcpyHostToDevice, h->stream));
        if (int rc = enqueue_forward(h, net.D, p, c.n_m, f.d_idx + c.idx0, c.B, false, w)) return rc;
        launch_fit_scatter_y(h->stream, c.n_m, w.act + p.h_off[L - 1], f.d_idx + c.idx0, f.d_len + c.m0, h->dataset.old(), c.B, (int64_t)p.act);
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    HIPCHECK(hipStreamSynchronize(h->stream));      // (the host tables the uploads read go out of scope)
    for (int64_t i = 0; i < n; i++) if (member_of_row[i] >= 0) h->dataset.h_old_set[(size_t)(first + i)] = 1;
    return 0;
}

// ---- advantages and value targets on the device (cloth_fit_gae.hpp has the definition and the order) ------------------------------------
extern "C" int clothhip_fit_data_gae(clothhip_handle *h, int64_t first, int64_t n, const ClothGaeParams *p, float *adv_out, float *ret_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->val.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no value network on this handle: call clothhip_set_value_mlp first");
    if (int rc = check_range(h, first, n)) return rc;
    if (!p) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (!std::isfinite(p->gamma) || !std::isfinite(p->lambda) || !std::isfinite(p->w_scale))
        return fail(CLOTHHIP_EINVAL, "gamma %g, lambda %g, w_scale %g: all three are finite", p->gamma, p->lambda, (double)p->w_scale);
    if (p->gamma < 0.0 || p->gamma > 1.0 || p->lambda < 0.0 || p->lambda > 1.0)
        return fail(CLOTHHIP_EINVAL, "gamma %g, lambda %g: both lie in [0, 1]", p->gamma, p->lambda);
    if (p->flags & ~(CLOTHHIP_GAE_WRITE_WEIGHTS | CLOTHHIP_GAE_NORMALIZE)) return fail(CLOTHHIP_EINVAL, "unknown flags 0x%x", p->flags);
    auto &f = h->fit;
    const auto &d = h->dataset;
    for (int64_t i = 0; i < n; i++) {
        const int32_t nx = d.h_next[(size_t)(first + i)];      // (greater than first + i where it is a row: clothhip_fit_data_set_transitions)
        if (nx >= 0 && nx >= first + n)
            return fail(CLOTHHIP_EINVAL, "row %lld: its successor %d lies outside the rows [%lld, %lld + %lld)", (long long)(first + i), nx, (long long)first, (long long)first, (long long)n);
    }
    if (n == 0) return 0;
    std::vector<int32_t> idx;
    try { idx.resize((size_t)n); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)n); }
    for (int64_t i = 0; i < n; i++) idx[(size_t)i] = (int32_t)(first + i);
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = f.d_gae_a.reserve((size_t)n * 8)) return rc;
    if (int rc = f.d_gae_stat.reserve(16)) return rc;
    if (int rc = f.d_adv.reserve((size_t)n * 4)) return rc;
    if (int rc = enqueue_predict(h, value_net(h), SHARED_ROW, 1, idx.data(), n, nullptr)) return rc;      // (records ev0; the scan moves ev1 behind itself)
    const bool write_w = (p->flags & CLOTHHIP_GAE_WRITE_WEIGHTS) != 0, normalize = (p->flags & CLOTHHIP_GAE_NORMALIZE) != 0;
    GaeArgs a = {};
    a.v = f.d_pred; a.rew = d.rew(); a.next = d.next(); a.ret = d.ret(); a.w = d.w(); a.A = f.d_gae_a; a.adv = f.d_adv; a.stat = f.d_gae_stat;
    a.first = first; a.n = n; a.gamma = p->gamma; a.c = p->gamma * p->lambda; a.w_scale = (double)p->w_scale; a.normalize = normalize ? 1 : 0;
    const dim3 grid((unsigned)((n + GAE_THREADS - 1) / GAE_THREADS));
    hipLaunchKernelGGL(k_gae_rows, grid, dim3(GAE_THREADS), 0, h->stream, a);
    HIPCHECK(hipGetLastError());
    if (write_w) {
        if (normalize) {
            hipLaunchKernelGGL(k_gae_stats, dim3(1), dim3(GAE_THREADS), 0, h->stream, a);
            HIPCHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_gae_weights, grid, dim3(GAE_THREADS), 0, h->stream, a);
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    if (adv_out) HIPCHECK(hipMemcpyAsync(adv_out, f.d_adv, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    if (ret_out) HIPCHECK(hipMemcpyAsync(ret_out, d.ret() + (size_t)first, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));      // (idx, a host table the upload read, goes out of scope)
    return 0;
}
