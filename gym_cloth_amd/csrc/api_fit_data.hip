// api_fit_data.hip -- the device-resident dataset of the trainer (api_fit.hip): its columns (api_handle.hpp: FIT_COL), how they grow, the host's
// range reads and writes of each, and the rows appended from where they lie on the device (held rows, the last launch's tables).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <initializer_list>
#include <new>
#include <utility>
#include <vector>

#include "api_handle.hpp"
#include "cloth_fit_gather.hpp"

static_assert(FIT_SRC_SLOTS == CLOTHHIP_FIT_SRC_SLOTS && FIT_SRC_RESETS == CLOTHHIP_FIT_SRC_RESETS && FIT_SRC_HELD == CLOTHHIP_FIT_SRC_HELD,
              "the row sources of the header and of the kernel");

// ---- the columns (clothhip.h: clothhip_fit_data_*) --------------------------------------------------------------------------------------
// where row `row` of column c lies
static uint32_t *col_at(const clothhip_handle *h, int c, int64_t row) { return h->dataset.col[c] + (size_t)row * FIT_COL[c].width(h->P); }
static size_t col_bytes(const clothhip_handle *h, int c, int64_t rows) { return (size_t)rows * FIT_COL[c].width(h->P) * 4; }

// room for n more rows: grow geometrically into new tables, keep the rows (Buffer::reserve would not), swap them in
static int grow_dataset(clothhip_handle *h, int64_t n) {
    auto &d = h->dataset;
    if (d.n + n <= d.cap) return 0;
    const int64_t cap = std::max<int64_t>(std::max<int64_t>(d.n + n, 2 * d.cap), 64);
    Buffer<uint32_t> grown[FIT_COLS];
    for (int c = 0; c < FIT_COLS; c++)
        if (int rc = grown[c].reserve(col_bytes(h, c, cap))) return rc;
    if (d.n > 0) {
        for (int c = 0; c < FIT_COLS; c++) HIPCHECK(hipMemcpyAsync(grown[c], d.col[c], col_bytes(h, c, d.n), hipMemcpyDeviceToDevice, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
    }
    for (int c = 0; c < FIT_COLS; c++) d.col[c] = std::move(grown[c]);
    d.cap = cap;
    return 0;
}

// The n rows behind the ones that count get the defaults of every column that has one (reward 0, no successor: a leaf, value target 0,
// old mean and old log sigma zeros), on the device, and the host mirrors theirs (no successor, neither old column set); enqueued, the caller synchronises before
// the rows count. After grow_dataset.
static int default_rows(clothhip_handle *h, int64_t n) {
    auto &d = h->dataset;
    try {
        d.h_next.resize((size_t)d.n); d.h_next.resize((size_t)(d.n + n), CLOTHHIP_FIT_NEXT_NONE);
        d.h_old_set.resize((size_t)d.n); d.h_old_set.resize((size_t)(d.n + n), 0);
        d.h_old_ls_set.resize((size_t)d.n); d.h_old_ls_set.resize((size_t)(d.n + n), 0);
    } catch (const std::bad_alloc &) {
        return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)(d.n + n));
    }
    for (int c = 0; c < FIT_COLS; c++)
        if (FIT_COL[c].defaulted) HIPCHECK(hipMemsetD32Async((hipDeviceptr_t)col_at(h, c, d.n), (int)FIT_COL[c].fill, col_bytes(h, c, n) / 4, h->stream));
    return 0;
}

// the rows [first, first + n) of a call lie within the dataset
int clothhip::check_range(const clothhip_handle *h, int64_t first, int64_t n) {
    if (first < 0 || n < 0 || first > h->dataset.n || n > h->dataset.n - first)
        return fail(CLOTHHIP_EINVAL, "rows [%lld, %lld + %lld) outside the dataset's %lld", (long long)first, (long long)first, (long long)n, (long long)h->dataset.n);
    return 0;
}

// The range writer of every clothhip_fit_data_set_*: what they all refuse, in their one order, then check() on the caller's values, then
// rows [first, first + n) of each column named from its host table, synchronously (the host tables are not retained). timed: the
// uploads lie between the timing events.
template <typename Check>
static int write_rows(clothhip_handle *h, int64_t first, int64_t n, std::initializer_list<std::pair<FitCol, const void *>> cols, Check check, bool timed = false) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (int rc = check_range(h, first, n)) return rc;
    if (n == 0) return 0;
    for (const auto &c : cols)
        if (!c.second) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check()) return rc;
    HIPCHECK(hipSetDevice(h->device));
    if (timed) HIPCHECK(hipEventRecord(h->ev0, h->stream));
    for (const auto &c : cols) HIPCHECK(hipMemcpyAsync(col_at(h, c.first, first), c.second, col_bytes(h, c.first, n), hipMemcpyHostToDevice, h->stream));
    if (timed) {
        HIPCHECK(hipEventRecord(h->ev1, h->stream));
        h->have_timing = true;
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// The range reader of every clothhip_fit_data_get*: the same refusals, then the rows of each column named into its host table.
// optional: a NULL table is skipped, not refused.
static int read_rows(clothhip_handle *h, int64_t first, int64_t n, std::initializer_list<std::pair<FitCol, void *>> cols, bool optional = false) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (int rc = check_range(h, first, n)) return rc;
    if (n == 0) return 0;
    bool any = false;
    for (const auto &c : cols) {
        if (!c.second && !optional) return fail(CLOTHHIP_EINVAL, "NULL argument");
        any = any || c.second;
    }
    if (!any) return 0;
    HIPCHECK(hipSetDevice(h->device));
    for (const auto &c : cols)
        if (c.second) HIPCHECK(hipMemcpyAsync(c.second, col_at(h, c.first, first), col_bytes(h, c.first, n), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// every value of a caller's table [n][width] a finite float, or the refusal that names the first one that is not: what[i], or
// what[row][column] for a table wider than one
static int check_finite(const float *v, int64_t n, int64_t width, const char *what) {
    for (int64_t i = 0; i < n * width; i++)
        if (!std::isfinite(v[i]))
            return width > 1 ? fail(CLOTHHIP_EINVAL, "%s[%lld][%lld] is not finite", what, (long long)(i / width), (long long)(i % width))
                             : fail(CLOTHHIP_EINVAL, "%s[%lld] is not finite", what, (long long)i);
    return 0;
}
// a caller's weight table (NULL: none given, which every entry that takes one allows)
static int check_weights(const float *w, int64_t n) { return w ? check_finite(w, n, 1, "weights") : 0; }

// The two searches of an append, host route or device route: the observations [n][3P], then the labels [n][4] as floats
static int check_obs_rows(const float *obs, int64_t n, int P) { return check_finite(obs, n, (int64_t)3 * P, "obs_rows"); }
static int check_label_rows(const float *lab, size_t n) {
    for (size_t i = 0; i < n * 4; i++)
        if (!std::isfinite(lab[i])) return fail(CLOTHHIP_EINVAL, "labels[%zu][%zu] is not a finite float (a slot that did not run? pass the rows that ran)", i / 4, i % 4);
    return 0;
}

extern "C" int clothhip_fit_data_append(clothhip_handle *h, const float *obs_rows, const double *labels, int64_t n) {
    return clothhip_fit_data_append_weighted(h, obs_rows, labels, nullptr, n);
}

extern "C" int clothhip_fit_data_append_weighted(clothhip_handle *h, const float *obs_rows, const double *labels, const float *weights, int64_t n) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (n < 0) return fail(CLOTHHIP_EINVAL, "n < 0");
    if (n == 0) return 0;
    if (!obs_rows || !labels) return fail(CLOTHHIP_EINVAL, "NULL argument");
    auto &d = h->dataset;
    if (d.n + n > INT32_MAX) return fail(CLOTHHIP_EINVAL, "%lld + %lld rows: a minibatch names its rows by int32", (long long)d.n, (long long)n);
    if (int rc = check_obs_rows(obs_rows, n, h->P)) return rc;
    std::vector<float> lab;
    try { lab.resize((size_t)n * 4); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld labels)", (long long)n); }
    for (size_t i = 0; i < (size_t)n * 4; i++) lab[i] = (float)labels[i];
    if (int rc = check_label_rows(lab.data(), (size_t)n)) return rc;
    if (int rc = check_weights(weights, n)) return rc;
    std::vector<float> ones;
    if (!weights) {
        try { ones.assign((size_t)n, 1.0f); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld weights)", (long long)n); }
        weights = ones.data();
    }
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = grow_dataset(h, n)) return rc;
    if (int rc = default_rows(h, n)) return rc;
    HIPCHECK(hipMemcpyAsync(col_at(h, COL_OBS, d.n), obs_rows, col_bytes(h, COL_OBS, n), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(col_at(h, COL_LAB, d.n), lab.data(), col_bytes(h, COL_LAB, n), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(col_at(h, COL_W, d.n), weights, col_bytes(h, COL_W, n), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));      // the host tables are never retained; only now do the rows count
    d.n += n;
    return 0;
}

extern "C" int clothhip_fit_data_set_weights(clothhip_handle *h, int64_t first, int64_t n, const float *w) {
    return write_rows(h, first, n, {{COL_W, w}}, [=] { return check_weights(w, n); }, true);
}

extern "C" int clothhip_fit_data_get_weights(clothhip_handle *h, int64_t first, int64_t n, float *w) { return read_rows(h, first, n, {{COL_W, w}}); }

// ---- the episode structure and the value targets (clothhip.h: ACTOR-CRITIC FROM REWARD) ---------------------------------------------------
extern "C" int clothhip_fit_data_set_transitions(clothhip_handle *h, int64_t first, int64_t n, const float *rew, const int32_t *next) {
    auto check = [=] {
        for (int64_t i = 0; i < n; i++) {
            if (!std::isfinite(rew[i])) return fail(CLOTHHIP_EINVAL, "rew[%lld] is not finite", (long long)i);
            const int64_t nx = next[i];
            if (nx != CLOTHHIP_FIT_NEXT_TERMINAL && nx != CLOTHHIP_FIT_NEXT_NONE && (nx <= first + i || nx >= h->dataset.n))
                return fail(CLOTHHIP_EINVAL, "next[%lld] = %lld: a successor lies behind its row %lld and inside the dataset's %lld (or CLOTHHIP_FIT_NEXT_TERMINAL, CLOTHHIP_FIT_NEXT_NONE)",
                            (long long)i, (long long)nx, (long long)(first + i), (long long)h->dataset.n);
        }
        return 0;
    };
    if (int rc = write_rows(h, first, n, {{COL_REW, rew}, {COL_NEXT, next}}, check)) return rc;
    std::copy(next, next + n, h->dataset.h_next.begin() + first);      // (the mirror follows the device)
    return 0;
}

extern "C" int clothhip_fit_data_get_transitions(clothhip_handle *h, int64_t first, int64_t n, float *rew, int32_t *next) {
    return read_rows(h, first, n, {{COL_REW, rew}, {COL_NEXT, next}});
}

extern "C" int clothhip_fit_data_set_returns(clothhip_handle *h, int64_t first, int64_t n, const float *ret) {
    return write_rows(h, first, n, {{COL_RET, ret}}, [=] { return check_finite(ret, n, 1, "ret"); });
}

extern "C" int clothhip_fit_data_get_returns(clothhip_handle *h, int64_t first, int64_t n, float *ret) { return read_rows(h, first, n, {{COL_RET, ret}}); }

// ---- the old means of PPO (clothhip.h: PPO ON THE DEVICE; clothhip_fit_data_snapshot_policy is the trainer's) ---------------------------
extern "C" int clothhip_fit_data_set_old_means(clothhip_handle *h, int64_t first, int64_t n, const float *mu) {
    if (int rc = write_rows(h, first, n, {{COL_OLD, mu}}, [=] { return check_finite(mu, n, 4, "mu"); })) return rc;
    h->dataset.mark_old_set(first, n);
    return 0;
}

// (an unset row holds zeros)
extern "C" int clothhip_fit_data_get_old_means(clothhip_handle *h, int64_t first, int64_t n, float *mu) { return read_rows(h, first, n, {{COL_OLD, mu}}); }

// ---- the old log sigma of PPO with a learned head (clothhip.h: PPO WITH A LEARNED SIGMA): the host route of the column ---------------------
extern "C" int clothhip_fit_data_set_old_log_sigma(clothhip_handle *h, int64_t first, int64_t n, const float *ls) {
    if (int rc = write_rows(h, first, n, {{COL_OLD_LS, ls}}, [=] { return check_finite(ls, n, 4, "ls"); })) return rc;
    h->dataset.mark_old_ls_set(first, n);
    return 0;
}

// (an unset row holds zeros)
extern "C" int clothhip_fit_data_get_old_log_sigma(clothhip_handle *h, int64_t first, int64_t n, float *ls) { return read_rows(h, first, n, {{COL_OLD_LS, ls}}); }

extern "C" int clothhip_fit_data_clear(clothhip_handle *h) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    h->dataset.n = 0;
    h->dataset.h_next.clear();
    h->dataset.h_old_set.clear();
    h->dataset.h_old_ls_set.clear();
    return 0;
}

extern "C" int clothhip_fit_data_size(clothhip_handle *h, int64_t *n) {
    if (!h || !n) return fail(CLOTHHIP_EINVAL, "NULL argument");
    *n = h->dataset.n;
    return 0;
}

extern "C" int clothhip_fit_data_get(clothhip_handle *h, int64_t first, int64_t n, float *obs, float *labels) {
    return read_rows(h, first, n, {{COL_OBS, obs}, {COL_LAB, labels}}, true);
}

// ---- the expert-action column of DDPG from demonstrations (clothhip.h: DDPG FROM DEMONSTRATIONS) ---------------------------------------
// a row is four finite values, or four NaNs: "no expert action", stored as the column's fill pattern whatever NaN was passed
extern "C" int clothhip_fit_data_set_expert(clothhip_handle *h, int64_t first, int64_t n, const float *a) {
    std::vector<uint32_t> bits;
    auto check = [&] {
        for (int64_t i = 0; i < n; i++) {
            int nans = 0;
            for (int k = 0; k < 4; k++) {
                const float v = a[4 * i + k];
                if (std::isinf(v)) return fail(CLOTHHIP_EINVAL, "a[%lld][%d] is infinite", (long long)i, k);
                nans += std::isnan(v) ? 1 : 0;
            }
            if (nans != 0 && nans != 4) return fail(CLOTHHIP_EINVAL, "a[%lld] mixes NaN and finite values: a row is four finite values, or four NaNs (no expert action)", (long long)i);
            for (int k = 0; k < 4; k++) {
                if (nans) bits[(size_t)(4 * i + k)] = FIT_COL[COL_EXP].fill;
                else memcpy(&bits[(size_t)(4 * i + k)], &a[4 * i + k], 4);
            }
        }
        return 0;
    };
    // the table uploaded is `bits`, which check() fills: write_rows takes the pointer before it runs check(), so the room is made here,
    // for a range that write_rows will accept
    if (h && a && first >= 0 && n > 0 && first <= h->dataset.n && n <= h->dataset.n - first) { try { bits.resize((size_t)n * 4); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)n); } }
    return write_rows(h, first, n, {{COL_EXP, a ? (const void *)bits.data() : nullptr}}, check);
}

extern "C" int clothhip_fit_data_get_expert(clothhip_handle *h, int64_t first, int64_t n, float *a) { return read_rows(h, first, n, {{COL_EXP, a}}); }

// ---- rows named by where they lie on the device (cloth_fit_gather.hpp) ------------------------------------------------------------------
// One (source, row) of a caller's table against what the handle holds now; the launch tables are valid under launch_table's rule.
static int check_source(const clothhip_handle *h, int64_t i, int32_t src, int32_t row) {
    int64_t rows = 0;
    switch (src) {
    case CLOTHHIP_FIT_SRC_SLOTS:
        if (int rc = launch_table(h, LaunchTable::obs, nullptr, &rows)) return rc;
        break;
    case CLOTHHIP_FIT_SRC_RESETS:
        if (int rc = launch_table(h, LaunchTable::reset_obs, nullptr, &rows)) return rc;
        break;
    case CLOTHHIP_FIT_SRC_HELD:
        if (!h->dataset.held_valid) return fail(CLOTHHIP_ESTATE, "no held rows on this handle: call clothhip_fit_hold first");
        rows = h->E;
        break;
    default:
        return fail(CLOTHHIP_EINVAL, "entry %lld: unknown row source %d", (long long)i, src);
    }
    if (row < 0 || row >= rows) return fail(CLOTHHIP_EINVAL, "entry %lld: row %d outside [0, %lld) of source %d", (long long)i, row, (long long)rows, src);
    return 0;
}

// upload n index entries [n][4] and run k_fit_gather over them; *bad: the kernel met a value that is not finite. label_src < 0: no
// entry names a label and no weight is written (the held rows), else CLOTHHIP_FIT_LABEL_* and dst_w gets `weights` [n] (host; NULL:
// ones). Synchronous.
static int run_gather(clothhip_handle *h, const std::vector<int32_t> &tab, int64_t n, float *dst_obs, float *dst_lab, float *dst_w, int32_t label_src,
                      const float *weights, bool *bad, float *dst_exp = nullptr) {
    auto &d = h->dataset;
    if (int rc = d.d_rows.reserve((size_t)n * 16)) return rc;
    if (int rc = d.d_flag.reserve(4)) return rc;
    if (weights) {
        if (int rc = d.d_wtab.reserve((size_t)n * 4)) return rc;
        HIPCHECK(hipMemcpyAsync(d.d_wtab, weights, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHECK(hipMemcpyAsync(d.d_rows, tab.data(), (size_t)n * 16, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemsetAsync(d.d_flag, 0, 4, h->stream));
    FitGatherArgs a = {};
    a.table[FIT_SRC_SLOTS] = (const float *)h->epi.d_fobs; a.table[FIT_SRC_RESETS] = (const float *)h->epi.d_frobs; a.table[FIT_SRC_HELD] = d.d_held;
    a.rows = d.d_rows;
    // (ACTION_EXPERT: both tables -- the record's action is the label, the label table's row goes to dst_exp)
    a.labels = label_src == CLOTHHIP_FIT_LABEL_EXPERT || label_src == CLOTHHIP_FIT_LABEL_ACTION_EXPERT ? (const double *)h->epi.d_flab : nullptr;
    a.records = label_src == CLOTHHIP_FIT_LABEL_ACTION || label_src == CLOTHHIP_FIT_LABEL_ACTION_EXPERT ? (const unsigned char *)(const void *)h->epi.d_frec : nullptr;
    a.dst_exp = dst_exp;
    a.weights = weights ? (const float *)d.d_wtab : nullptr;
    a.dst_obs = dst_obs; a.dst_lab = dst_lab; a.dst_w = dst_w; a.flag = d.d_flag; a.n = n; a.L = 3 * h->P;
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(k_fit_gather, dim3((unsigned)std::min<int64_t>(n, 1 << 20)), dim3(FIT_GATHER_THREADS), 0, h->stream, a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    int32_t flag = 0;
    HIPCHECK(hipMemcpyAsync(&flag, d.d_flag, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    *bad = flag != 0;
    return 0;
}

// The refusal of an append whose kernel raised the flag, with clothhip_fit_data_append's message: what the kernel wrote behind the rows
// that count is read back and searched in that entry's order (observations first, then the rounded labels).
static int bad_value(clothhip_handle *h, int64_t n, bool expert) {
    const size_t row = (size_t)3 * h->P;
    std::vector<float> buf;
    try { buf.resize((size_t)n * std::max<size_t>(row, 4)); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_EINVAL, "an observation or a label is not a finite float"); }
    HIPCHECK(hipMemcpy(buf.data(), col_at(h, COL_OBS, h->dataset.n), col_bytes(h, COL_OBS, n), hipMemcpyDeviceToHost));
    if (int rc = check_obs_rows(buf.data(), n, h->P)) return rc;
    HIPCHECK(hipMemcpy(buf.data(), col_at(h, COL_LAB, h->dataset.n), col_bytes(h, COL_LAB, n), hipMemcpyDeviceToHost));
    if (int rc = check_label_rows(buf.data(), (size_t)n)) return rc;
    if (expert) {
        HIPCHECK(hipMemcpy(buf.data(), col_at(h, COL_EXP, h->dataset.n), col_bytes(h, COL_EXP, n), hipMemcpyDeviceToHost));
        if (int rc = check_finite(buf.data(), n, 4, "expert")) return rc;
    }
    return fail(CLOTHHIP_EINVAL, "an observation or a label is not a finite float");
}

extern "C" int clothhip_fit_hold(clothhip_handle *h, const int32_t *src) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    auto &d = h->dataset;
    const size_t row = (size_t)3 * h->P;
    std::vector<int32_t> tab;
    if (src) {
        for (int e = 0; e < h->E; e++) {
            const int32_t s = src[2 * e], r = src[2 * e + 1];
            if (int rc = check_source(h, e, s, r)) return rc;
            if (s == CLOTHHIP_FIT_SRC_HELD) {     // only its own row, which stays: another env's may be overwritten by this very call
                if (r != e) return fail(CLOTHHIP_EINVAL, "entry %d: a held row can only be kept (row %d), not moved to another env", e, r);
                continue;
            }
            try { tab.insert(tab.end(), {s, r, -1, (int32_t)e}); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory"); }
        }
    }
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = d.d_held.reserve((size_t)h->E * row * 4)) return rc;      // (no earlier contents to keep: a table named HELD rows only if it existed)
    if (!src) {
        if (int rc = clothhip_write_obs_f32_device(h, d.d_held)) return rc;
        HIPCHECK(hipStreamSynchronize(h->stream));
    } else if (!tab.empty()) {
        bool bad = false;      // (a held row is not checked here: clothhip_fit_data_append_launch checks what it appends)
        if (int rc = run_gather(h, tab, (int64_t)tab.size() / 4, d.d_held, nullptr, nullptr, -1, nullptr, &bad)) return rc;
    }
    d.held_valid = true;
    return 0;
}

extern "C" int clothhip_fit_data_append_launch(clothhip_handle *h, const int32_t *rows, int64_t n) {
    return clothhip_fit_data_append_launch_ex(h, rows, n, CLOTHHIP_FIT_LABEL_EXPERT, nullptr);
}

static_assert(sizeof(ClothStepRecord) == FIT_REC_BYTES && offsetof(ClothStepRecord, action) == 0 && offsetof(ClothStepRecord, ran) == FIT_REC_RAN,
              "the record's layout as k_fit_gather reads it");

extern "C" int clothhip_fit_data_append_launch_ex(clothhip_handle *h, const int32_t *rows, int64_t n, int32_t label_src, const float *weights) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    const bool both = label_src == CLOTHHIP_FIT_LABEL_ACTION_EXPERT;      // the executed action as the label AND the expert's into its column
    if (label_src != CLOTHHIP_FIT_LABEL_EXPERT && label_src != CLOTHHIP_FIT_LABEL_ACTION && label_src != CLOTHHIP_FIT_LABEL_ZERO && !both)
        return fail(CLOTHHIP_EINVAL, "unknown label source %d (CLOTHHIP_FIT_LABEL_EXPERT, CLOTHHIP_FIT_LABEL_ACTION, CLOTHHIP_FIT_LABEL_ZERO or CLOTHHIP_FIT_LABEL_ACTION_EXPERT)", label_src);
    const bool zero = label_src == CLOTHHIP_FIT_LABEL_ZERO;      // no label table is read: label_row is ignored (the kernel is told row 0 of no table)
    if (n < 0) return fail(CLOTHHIP_EINVAL, "n < 0");
    if (n == 0) return 0;
    if (!rows) return fail(CLOTHHIP_EINVAL, "NULL argument");
    auto &d = h->dataset;
    if (d.n + n > INT32_MAX) return fail(CLOTHHIP_EINVAL, "%lld + %lld rows: a minibatch names its rows by int32", (long long)d.n, (long long)n);
    int64_t n_lab = 0;
    if (!zero) if (int rc = launch_table(h, label_src == CLOTHHIP_FIT_LABEL_ACTION ? LaunchTable::records : LaunchTable::labels, nullptr, &n_lab)) return rc;
    if (both) {      // (both tables have T * E rows)
        int64_t n_rec = 0;
        if (int rc = launch_table(h, LaunchTable::records, nullptr, &n_rec)) return rc;
        n_lab = std::min(n_lab, n_rec);
    }
    if (int rc = check_weights(weights, n)) return rc;
    std::vector<int32_t> tab;
    try { tab.resize((size_t)n * 4); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)n); }
    for (int64_t i = 0; i < n; i++) {
        const int32_t s = rows[3 * i], r = rows[3 * i + 1], l = rows[3 * i + 2];
        if (int rc = check_source(h, i, s, r)) return rc;
        if (!zero && (l < 0 || l >= n_lab)) return fail(CLOTHHIP_EINVAL, "entry %lld: label row %d outside [0, %lld)", (long long)i, l, (long long)n_lab);
        tab[4 * i] = s; tab[4 * i + 1] = r; tab[4 * i + 2] = zero ? 0 : l; tab[4 * i + 3] = (int32_t)(d.n + i);
    }
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = grow_dataset(h, n)) return rc;
    if (int rc = default_rows(h, n)) return rc;
    // the kernel writes behind the n rows that count; they count only if every value it wrote is finite
    bool bad = false;
    if (int rc = run_gather(h, tab, n, d.obs(), d.lab(), d.w(), label_src, weights, &bad, both ? d.expert() : nullptr)) return rc;
    if (bad) return bad_value(h, n, both);      // (what was written lies behind the rows that count: the next append's defaults overwrite it)
    d.n += n;
    return 0;
}

// ---- the three kernels of cloth_fit_gather.hpp that the trainer enqueues (a header with a non-template kernel has one includer) -----------
void clothhip::launch_fit_sqsum(hipStream_t s, const float *y, const float *lab, const float *wgt, const int32_t *rows, int32_t B, double *sum) {
    hipLaunchKernelGGL(k_fit_sqsum, dim3(1), dim3(256), 0, s, y, lab, wgt, rows, B, sum);
}
void clothhip::launch_fit_copy_y(hipStream_t s, int32_t n_m, const float *y, int32_t n_vals, float *out, int64_t y_step, int64_t out_step, int32_t blocks) {
    hipLaunchKernelGGL(k_fit_copy_y, dim3((unsigned)blocks * (unsigned)n_m), dim3(256), 0, s, y, n_vals, out, y_step, out_step, blocks);
}
void clothhip::launch_fit_scatter_y(hipStream_t s, int32_t n_m, const float *y, const int32_t *rows, const int32_t *len, float *col, int32_t B, int64_t y_step) {
    const int32_t blocks = (B + 255) / 256;
    hipLaunchKernelGGL(k_fit_scatter_y, dim3((unsigned)blocks * (unsigned)n_m), dim3(256), 0, s, y, rows, len, col, B, y_step, blocks);
}
