// pandrs_hip.hpp — C++17 host-side mirror of the reference's API for the accelerated path, over the
// C ABI of include/pandrs_hip.h (header only; link libpandrs_hip.so).
//
// The reference is a Rust crate and this image has no Rust toolchain, so this header plays the part of
// the crate-side shim in a compiled language: same type and method names, argument meaning and error
// behaviour as
//   OptimizedDataFrame        src/optimized/split_dataframe/core.rs, group/grouping.rs:22-115,
//                             join.rs:32-73, aggregate.rs:21-217, sort.rs:18-272, data_ops.rs:15-121,
//                             row_ops.rs:26-130, parallel.rs:21-230, select.rs:150-167;
//                             rolling / expanding / ewm: src/dataframe/window.rs:13-160 (series/window.rs)
//                             rolling_median: pandas_compat/helpers/window_ops.rs:206-240; apply_rolling / apply_expanding
//                             (median, quantile and the other operations): src/dataframe/enhanced_window.rs
//                             describe / describe_all: src/optimized/split_dataframe/stats.rs:50-171
//                             rank: src/dataframe/pandas_compat/functions.rs:193-236
//                             nlargest / nsmallest / idxmax / idxmin: functions.rs:159-192
//                             value_range / cut / qcut: functions.rs:2270-2282, :2339-2420
//                             value_counts / unique / nunique / mode_* / is_unique: functions.rs:343-384, :775-788, :1709-1753, :4120-4139, :4226-4259
//                             crosstab / pivot / unstack: functions.rs:2138-2183, :2471-2527; pivot_table / AggFunction: src/pivot/mod.rs:12-250
//                             gt / ge / lt / le / eq_value / ne_value: pandas_compat/helpers/comparison_ops.rs:7-46;
//                             between / is_between / isna / notna / is_finite / is_infinite / isin / isin_numeric /
//                             query_* / dropna / count_na / has_nulls / count_value: functions.rs:141-158, :253-257,
//                             :920-933, :1312-1315, :2776-2795, :3837-3840, :4016-4024, :4089-4095, :4141-4161, :4187-4190
//   Column / *Column          src/column/{int64,float64,string,boolean}_column.rs, core/column.rs:163-177
//   GroupBy, AggregateOp      group/types.rs:11-55, group/aggregation.rs:763-871, group/operations.rs:438-547
//   LazyFrame                 src/optimized/lazy.rs:98-170, :186-425
//   JoinType                  join.rs:11-20
//   Error                     src/core/error.rs:6 (Result<T, Error> becomes: returns T, throws Error)
// Everything numeric happens in the library (host pointers, PANDRS_HIP_MEM_HOST — the way the Rust shim
// of INTEGRATION.md calls it); this header only stringifies keys, names columns and assembles frames,
// exactly the host-side work the reference keeps.  tests/cpp/reference_like_tests.cpp replays the
// reference's own tests through it.
#pragma once
#include <algorithm>
#include <cctype>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <variant>
#include <vector>

#include "pandrs_hip.h"

namespace pandrs {

// ---- errors (src/core/error.rs) ---------------------------------------------------------------------
struct Error : std::runtime_error {
    enum Kind { ColumnNotFound, ColumnTypeMismatch, OperationFailed, Computation, InvalidInput, DuplicateColumnName, InconsistentRowCount, Empty, Type, BelowThreshold, Index,
                EmptyColumnList, InconsistentArrayLengths,     // sort.rs:147-149, :161-166
                Format,                                        // select.rs:151-157 (select_by_mask's mask length)
                InvalidValue };                                // series/window.rs:113-116, :567-573, dataframe/window.rs:62-67, stats/descriptive.rs:92-96
    Kind kind;
    Error(Kind k, const std::string &m) : std::runtime_error(m), kind(k) {}
};

namespace detail {
// device failures map like src/gpu/mod.rs:206-210
inline void check(int32_t st) {
    if (st == PANDRS_HIP_OK) return;
    const std::string msg = pandrs_hip_last_error();
    switch (st) {
    case PANDRS_HIP_ERR_INVALID_ARGUMENT: throw Error(Error::InvalidInput, msg);
    case PANDRS_HIP_ERR_TYPE_MISMATCH: throw Error(Error::ColumnTypeMismatch, msg);
    case PANDRS_HIP_ERR_OPERATION_FAILED: throw Error(Error::OperationFailed, msg);
    case PANDRS_HIP_ERR_BELOW_THRESHOLD: throw Error(Error::BelowThreshold, msg);     // the shim keeps its CPU path (gpu.rs:30-32)
    default: throw Error(Error::Computation, msg);
    }
}
// process-wide context, created on first use (cf. get_gpu_manager, src/gpu/mod.rs:249-282)
inline pandrs_hip_ctx *context() {
    static std::once_flag once;
    static pandrs_hip_ctx *ctx = nullptr;
    std::call_once(once, [] {
        check(pandrs_hip_init(nullptr));
        check(pandrs_hip_ctx_create(0, &ctx));
    });
    return ctx;
}
// create_bitmask (src/core/column.rs:163-177): LSB first, 1 = null; empty when nothing is null
inline std::vector<uint8_t> create_bitmask(const std::vector<bool> &nulls) {
    bool any = false;
    for (bool b : nulls) any = any || b;
    if (!any) return {};
    std::vector<uint8_t> m((nulls.size() + 7) / 8, 0);
    for (size_t i = 0; i < nulls.size(); i++)
        if (nulls[i]) m[i >> 3] |= (uint8_t)(1u << (i & 7));
    return m;
}
inline bool bit_at(const std::vector<uint8_t> &m, size_t i) { return !m.empty() && ((m[i >> 3] >> (i & 7)) & 1); }
// f64::to_string(): shortest round-trip digits, never an exponent ("1", "0.1", "NaN", "inf", "-0")
inline std::string rust_f64_to_string(double v) {
    if (v != v) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char buf[400];
    auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}
}  // namespace detail

// ---- GLOBAL_STRING_POOL (src/column/string_pool.rs:28-53): equal string <=> equal code ----------------
class StringPool {
public:
    static StringPool &global() { static StringPool p; return p; }
    uint32_t get_or_insert(const std::string &s) {
        std::lock_guard<std::mutex> lock(mu_);
        auto it = codes_.find(s);
        if (it != codes_.end()) return it->second;
        const uint32_t c = (uint32_t)strings_.size();
        strings_.push_back(s);
        codes_.emplace(s, c);
        return c;
    }
    std::string get(uint32_t code) const {
        std::lock_guard<std::mutex> lock(mu_);
        return strings_.at(code);
    }
    // the code of a string the pool already holds; nullopt for one it has never seen (nothing is inserted)
    std::optional<uint32_t> find(const std::string &s) const {
        std::lock_guard<std::mutex> lock(mu_);
        auto it = codes_.find(s);
        if (it == codes_.end()) return std::nullopt;
        return it->second;
    }
    // rank[code] = position of the code's string in byte-wise order (Rust String: Ord; std::string compares its
    // chars as unsigned char): the table pandrs_hip_sort_indices orders string keys by
    std::vector<uint32_t> rank_table() const {
        std::lock_guard<std::mutex> lock(mu_);
        std::vector<uint32_t> order(strings_.size()), rank(strings_.size());
        for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return strings_[a] < strings_[b]; });
        for (size_t i = 0; i < order.size(); i++) rank[order[i]] = (uint32_t)i;
        return rank;
    }
private:
    mutable std::mutex mu_;
    std::vector<std::string> strings_;
    std::unordered_map<std::string, uint32_t> codes_;
};

// ---- columns ----------------------------------------------------------------------------------------------
struct Int64Column {          // src/column/int64_column.rs:52-66
    std::vector<int64_t> data;
    std::vector<uint8_t> null_mask;
    Int64Column() = default;
    explicit Int64Column(std::vector<int64_t> d) : data(std::move(d)) {}
    static Int64Column with_nulls(std::vector<int64_t> d, const std::vector<bool> &nulls) {
        Int64Column c(std::move(d)); c.null_mask = detail::create_bitmask(nulls); return c;
    }
    size_t len() const { return data.size(); }
};
struct Float64Column {        // src/column/float64_column.rs:9-13
    std::vector<double> data;
    std::vector<uint8_t> null_mask;
    Float64Column() = default;
    explicit Float64Column(std::vector<double> d) : data(std::move(d)) {}
    static Float64Column with_nulls(std::vector<double> d, const std::vector<bool> &nulls) {
        Float64Column c(std::move(d)); c.null_mask = detail::create_bitmask(nulls); return c;
    }
    size_t len() const { return data.size(); }
};
struct StringColumn {         // src/column/string_column.rs:26-72 (GlobalPool mode): pool codes
    std::vector<uint32_t> indices;
    std::vector<uint8_t> null_mask;
    StringColumn() = default;
    explicit StringColumn(const std::vector<std::string> &values) {
        indices.reserve(values.size());
        for (auto &s : values) indices.push_back(StringPool::global().get_or_insert(s));
    }
    static StringColumn with_nulls(const std::vector<std::string> &values, const std::vector<bool> &nulls) {
        StringColumn c(values); c.null_mask = detail::create_bitmask(nulls); return c;
    }
    size_t len() const { return indices.size(); }
    std::string get(size_t i) const { return StringPool::global().get(indices[i]); }
};
struct BooleanColumn {        // src/column/boolean_column.rs:10-15: LSB-first packed bits
    std::vector<uint8_t> bits;
    size_t length = 0;
    std::vector<uint8_t> null_mask;
    BooleanColumn() = default;
    explicit BooleanColumn(const std::vector<bool> &values) : bits((values.size() + 7) / 8, 0), length(values.size()) {
        for (size_t i = 0; i < values.size(); i++)
            if (values[i]) bits[i >> 3] |= (uint8_t)(1u << (i & 7));
    }
    size_t len() const { return length; }
    bool get(size_t i) const { return (bits[i >> 3] >> (i & 7)) & 1; }
};
using Column = std::variant<Int64Column, Float64Column, StringColumn, BooleanColumn>;

namespace detail {
inline size_t col_len(const Column &c) { return std::visit([](auto &x) { return x.len(); }, c); }
inline int32_t col_dtype(const Column &c) { return (int32_t)c.index(); }   // variant order == pandrs_hip_dtype order
inline pandrs_hip_column view(const Column &c) {
    pandrs_hip_column v{};
    v.dtype = col_dtype(c);
    std::visit([&](auto &x) {
        using T = std::decay_t<decltype(x)>;
        if constexpr (std::is_same_v<T, StringColumn>) v.data = x.indices.data();
        else if constexpr (std::is_same_v<T, BooleanColumn>) v.data = x.bits.data();
        else v.data = x.data.data();
        v.null_mask = x.null_mask.empty() ? nullptr : x.null_mask.data();
    }, c);
    return v;
}
// Columns uploaded once (pandrs_hip_column_upload) and shared by every copy of the frame: the stand-in for the Rust
// shim's ResidentCache over the reference's immutable Arc<[T]> columns (src/column/int64_column.rs:10), which the
// public frame's operators Arc-clone on every call (src/optimized/dataframe/transformations.rs:524-577, :628-694).
struct ResidentSet {
    std::vector<pandrs_hip_column> cols;
    ResidentSet() = default;
    ResidentSet(const ResidentSet &) = delete;
    ResidentSet &operator=(const ResidentSet &) = delete;
    ~ResidentSet() { for (auto &c : cols) (void)pandrs_hip_column_release(context(), &c); }
};
// a host table copied to HBM for one call whose columns are resident (the string rank table of a sort), freed after it
struct Staged {
    pandrs_hip_column dev{};
    const uint32_t *upload(const std::vector<uint32_t> &v) {
        pandrs_hip_column host{v.data(), nullptr, PANDRS_HIP_U32CODE, 0};
        check(pandrs_hip_column_upload(context(), &host, (int64_t)v.size(), &dev));
        return static_cast<const uint32_t *>(dev.data);
    }
    ~Staged() { if (dev.data) (void)pandrs_hip_column_release(context(), &dev); }
};
// group-key cell -> the string the reference's result frame holds (grouping.rs:69-98)
inline std::string key_string(int32_t dtype, uint64_t cell, bool is_null, const char *null_string = "NULL") {
    if (is_null) return null_string;
    switch (dtype) {
    case PANDRS_HIP_I64: return std::to_string((int64_t)cell);
    case PANDRS_HIP_F64: { double d; std::memcpy(&d, &cell, 8); return rust_f64_to_string(d); }
    case PANDRS_HIP_U32CODE: return StringPool::global().get((uint32_t)cell);
    default: return cell ? "true" : "false";
    }
}
}  // namespace detail

// RankMethod (src/dataframe/pandas_compat/types.rs:48-59), same order: the values of pandrs_hip_rank_method
enum class RankMethod : int32_t { Average = 0, Min = 1, Max = 2, First = 3, Dense = 4 };

// StatDescribe (src/optimized/split_dataframe/stats.rs:13-19): count, mean, std, min, 25%, 50%, 75%, max
struct StatDescribe {
    std::unordered_map<std::string, double> stats;
    std::vector<std::pair<std::string, double>> stats_list;    // the same, in that order
};

enum class AggregateOp { Sum = 0, Mean, Min, Max, Count, Std, Var, Median, First, Last, Custom,   // types.rs:11-34
                         Nunique };   // + the legacy AggFunc::Nunique (src/dataframe/groupby.rs:41)
enum class JoinType { Inner = 0, Left, Right, Outer };                                              // join.rs:11-20
// AggFunction (src/pivot/mod.rs:12-48), same order; agg_function_name / agg_function_from_str are its name() / from_str()
enum class AggFunction { Sum = 0, Mean, Min, Max, Count };
inline const char *agg_function_name(AggFunction f) {
    static const char *const names[] = {"sum", "mean", "min", "max", "count"};
    return names[(int)f];
}
inline bool agg_function_from_str(std::string s, AggFunction *out) {
    for (auto &ch : s) ch = (char)std::tolower((unsigned char)ch);
    if (s == "sum") *out = AggFunction::Sum;
    else if (s == "mean" || s == "avg" || s == "average") *out = AggFunction::Mean;
    else if (s == "min" || s == "minimum") *out = AggFunction::Min;
    else if (s == "max" || s == "maximum") *out = AggFunction::Max;
    else if (s == "count") *out = AggFunction::Count;
    else return false;
    return true;
}

class GroupBy;

// ---- the window builder (dataframe/enhanced_window.rs:14-75): configurations for apply_rolling / apply_expanding ----
struct DataFrameRolling {
    size_t window_size;
    int64_t min_periods_ = -1;                 // < 0: window_size (enhanced_window.rs:305)
    bool center_ = false, has_columns_ = false;
    std::vector<std::string> columns_;
    explicit DataFrameRolling(size_t w) : window_size(w) {}
    DataFrameRolling &min_periods(size_t m) { min_periods_ = (int64_t)m; return *this; }
    DataFrameRolling &center(bool c) { center_ = c; return *this; }
    DataFrameRolling &columns(std::vector<std::string> c) { columns_ = std::move(c); has_columns_ = true; return *this; }
};
struct DataFrameExpanding {
    size_t min_periods;
    bool has_columns_ = false;
    std::vector<std::string> columns_;
    explicit DataFrameExpanding(size_t m) : min_periods(m) {}
    DataFrameExpanding &columns(std::vector<std::string> c) { columns_ = std::move(c); has_columns_ = true; return *this; }
};
class DataFrameRollingOps;
class DataFrameExpandingOps;

// ---- OptimizedDataFrame ------------------------------------------------------------------------------------
class OptimizedDataFrame {
public:
    std::vector<Column> columns;
    std::vector<std::string> column_names;
    std::unordered_map<std::string, size_t> column_indices;
    // the StringMultiIndex a multi-key group_by(..).aggregate(..) sets instead of key columns (aggregation.rs:812-853,
    // split_dataframe/index.rs:94-111): one tuple of key strings per row, the level names = the grouping columns
    std::vector<std::vector<std::string>> multi_index;
    std::vector<std::string> multi_index_names;
    bool has_multi_index() const { return !multi_index_names.empty(); }

    OptimizedDataFrame &add_column(const std::string &name, Column column) {
        if (column_indices.count(name)) throw Error(Error::DuplicateColumnName, name);
        if (!columns.empty() && detail::col_len(column) != row_count_)
            throw Error(Error::InconsistentRowCount, "expected " + std::to_string(row_count_) + " rows, found " + std::to_string(detail::col_len(column)));
        row_count_ = detail::col_len(column);
        column_indices[name] = columns.size();
        column_names.push_back(name);
        columns.push_back(std::move(column));
        resident_.reset();                       // the device copies describe the frame as it was
        return *this;
    }
    // Uploads every column to HBM once; group_by(..).aggregate(..), groups(), joins, gathers and the whole-column
    // reductions of this frame AND its copies then read the device copies (PANDRS_HIP_MEM_DEVICE) instead of staging
    // the host vectors on every call.  The columns must not be modified afterwards (the reference's are immutable).
    OptimizedDataFrame &make_resident() {
        auto rs = std::make_shared<detail::ResidentSet>();
        rs->cols.reserve(columns.size());
        for (auto &c : columns) {
            pandrs_hip_column host = detail::view(c), dev{};
            detail::check(pandrs_hip_column_upload(detail::context(), &host, (int64_t)detail::col_len(c), &dev));
            rs->cols.push_back(dev);
        }
        resident_ = std::move(rs);
        return *this;
    }
    bool is_resident() const { return resident_ != nullptr; }
    // the column's view for a library call, and the memory space it lives in
    pandrs_hip_column view_of(const std::string &name) const {
        auto it = column_indices.find(name);
        if (it == column_indices.end()) throw Error(Error::ColumnNotFound, name);
        return resident_ ? resident_->cols[it->second] : detail::view(columns[it->second]);
    }
    int32_t mem_space() const { return resident_ ? PANDRS_HIP_MEM_DEVICE : PANDRS_HIP_MEM_HOST; }
    const Column &column(const std::string &name) const {
        auto it = column_indices.find(name);
        if (it == column_indices.end()) throw Error(Error::ColumnNotFound, name);
        return columns[it->second];
    }
    bool contains_column(const std::string &name) const { return column_indices.count(name) != 0; }
    size_t row_count() const { return row_count_; }
    size_t column_count() const { return columns.size(); }

    GroupBy group_by(const std::vector<std::string> &cols) const;                      // grouping.rs:22-28: as_multi_index = true
    GroupBy group_by_with_options(const std::vector<std::string> &cols, bool as_multi_index) const;   // grouping.rs:38-115
    std::map<std::string, OptimizedDataFrame> par_groupby(const std::vector<std::string> &cols) const;   // grouping.rs:124-331

    OptimizedDataFrame inner_join(const OptimizedDataFrame &o, const std::string &l, const std::string &r) const { return join_impl(o, l, r, JoinType::Inner); }
    OptimizedDataFrame left_join(const OptimizedDataFrame &o, const std::string &l, const std::string &r) const { return join_impl(o, l, r, JoinType::Left); }
    OptimizedDataFrame right_join(const OptimizedDataFrame &o, const std::string &l, const std::string &r) const { return join_impl(o, l, r, JoinType::Right); }
    OptimizedDataFrame outer_join(const OptimizedDataFrame &o, const std::string &l, const std::string &r) const { return join_impl(o, l, r, JoinType::Outer); }

    // whole-column reductions (split_dataframe/aggregate.rs:21-215): the non-null values as f64, sum 0.0 when
    // there is none, mean / min / max Err(Error::Empty) then; min / max fold with f64::min / f64::max from +-inf
    double sum(const std::string &name) const { return stats(name).sum_f64; }
    double mean(const std::string &name) const { auto s = non_empty(name); return s.sum_f64 / (double)s.count; }
    double min(const std::string &name) const { return non_empty(name).min; }
    double max(const std::string &name) const { return non_empty(name).max; }

    // describe (stats.rs:50-151 over stats/descriptive.rs:91-200): count, mean, std (two passes, count - 1), min, the
    // 25 / 50 / 75 percentiles (linear interpolation at (p / 100) * (count - 1)) and max of the non-null cells as f64, from
    // one pandrs_hip_describe call (a radix select, no sort).  Errors before any device call: ColumnNotFound, Type (a
    // String or Boolean column).  InvalidValue for a column without a non-null cell (descriptive.rs:92-96) and for one
    // with a single non-null cell (the reference's confidence interval refuses 0 degrees of freedom,
    // stats/distributions.rs:188-193).  NaN cells order after every number (pandrs_hip.h).
    StatDescribe describe(const std::string &column_name) const {
        const Column &c = column(column_name);
        if (c.index() > 1) throw Error(Error::Type, "Column '" + column_name + "' is not a numeric type");      // stats.rs:146-149
        pandrs_hip_describe_stats st{};
        if (row_count_) {
            const pandrs_hip_column v = view_of(column_name);
            detail::check(pandrs_hip_describe(detail::context(), mem_space(), &v, (int64_t)row_count_, &st));
        }
        if (st.count == 0) throw Error(Error::InvalidValue, "Cannot compute statistics for empty data");
        if (st.count == 1) throw Error(Error::InvalidValue, "Degrees of freedom must be positive");
        StatDescribe d;
        d.stats_list = {{"count", (double)st.count}, {"mean", st.mean}, {"std", st.std}, {"min", st.min},
                        {"25%", st.q1}, {"50%", st.median}, {"75%", st.q3}, {"max", st.max}};                  // stats.rs:74-83
        for (auto &kv : d.stats_list) d.stats[kv.first] = kv.second;
        return d;
    }
    // rank (PandasCompatExt::rank, src/dataframe/pandas_compat/functions.rs:193-236): the ascending 1-based rank of every row
    // of an Int64 or Float64 column from one pandrs_hip_rank call (the stable radix sort, tie-run boundaries, a scatter); a
    // tie run at sorted positions [s, e) ranks (s + e + 1) / 2 (Average), s + 1 (Min), e (Max), position + 1 in row order
    // (First) or the run's number (Dense).  Errors before any device call: ColumnNotFound, Type (a String or Boolean column).
    // A NaN or null cell gets NaN and takes no rank; Int64 cells are compared as integers (pandrs_hip.h).
    std::vector<double> rank(const std::string &column_name, RankMethod method = RankMethod::Average) const {
        const Column &c = column(column_name);
        if (c.index() > 1) throw Error(Error::Type, "Column '" + column_name + "' is not a numeric type");
        std::vector<double> ranks(row_count_);
        if (row_count_) {
            const pandrs_hip_column v = view_of(column_name);
            detail::check(pandrs_hip_rank(detail::context(), mem_space(), &v, (int64_t)row_count_, (int32_t)method,
                                          PANDRS_HIP_MEM_HOST, ranks.data()));
        }
        return ranks;
    }
    // nlargest / nsmallest (PandasCompatExt, src/dataframe/pandas_compat/functions.rs:159-174): the min(n, row_count()) rows with
    // the largest / smallest values of an Int64 or Float64 column, in that order, ties in row order, from one pandrs_hip_topk
    // call (a radix select, a compaction, a sort of fewer than n rows) - sort_by's first n rows without the sort.  The frame is
    // assembled as sort_by_columns assembles its own: nulls become 0 / 0.0 / "" / false, no masks, no columns when there are no
    // rows.  Errors before any device call: ColumnNotFound, Type (a String or Boolean column).  NaN rows, then null rows, come
    // after every number in both directions; Int64 cells are compared as integers (pandrs_hip.h).
    OptimizedDataFrame nlargest(size_t n, const std::string &column_name) const { return topk(n, column_name, PANDRS_HIP_TOPK_LARGEST); }
    OptimizedDataFrame nsmallest(size_t n, const std::string &column_name) const { return topk(n, column_name, PANDRS_HIP_TOPK_SMALLEST); }
    // idxmax / idxmin (functions.rs:175-192): the LAST row of the largest value (Iterator::max_by) / the FIRST row of the smallest
    // (min_by), NaN and null cells skipped; nullopt when the column holds no number.  One pandrs_hip_arg_extreme pass for both.
    std::optional<size_t> idxmax(const std::string &column_name) const { return arg_extreme(column_name, 1); }
    std::optional<size_t> idxmin(const std::string &column_name) const { return arg_extreme(column_name, 0); }
    // Shape statistics (PandasCompatExt: skew / kurtosis, src/dataframe/pandas_compat/functions.rs:1617-1665; sem / mad / prod / cv /
    // geometric_mean / harmonic_mean / iqr / percentile_value / trimmed_mean / describe_column, helpers/aggregations.rs:8-225;
    // var_column / std_column, functions.rs:3571-3588; range / abs_sum, :4207-4224; zscore, :2284-2314; the *_all lists, :934-1022,
    // :1583-1615).  Each is the reference's expression, early returns included, over the fields of ONE pandrs_hip_moments call
    // (asking only for the `want` bits it needs) and / or ONE pandrs_hip_order_stats call.  The cells that count are neither null
    // nor NaN.  Errors before any device call: ColumnNotFound, Type (a String or Boolean column).
    pandrs_hip_moments_stats moments(const std::string &column_name, uint32_t want) const {
        numeric(column_name);
        pandrs_hip_moments_stats st{};
        const pandrs_hip_column v = view_of(column_name);
        detail::check(pandrs_hip_moments(detail::context(), mem_space(), &v, 1, (int64_t)row_count_, want, &st));
        return st;
    }
    struct OrderStat { int32_t op; double arg; };
    std::pair<std::vector<double>, int64_t> order_stats(const std::string &column_name, const std::vector<OrderStat> &ops) const {
        numeric(column_name);
        std::vector<int32_t> op;
        std::vector<double> arg, out(ops.size());
        for (const OrderStat &o : ops) { op.push_back(o.op); arg.push_back(o.arg); }
        int64_t m = 0;
        const pandrs_hip_column v = view_of(column_name);
        detail::check(pandrs_hip_order_stats(detail::context(), mem_space(), &v, (int64_t)row_count_, op.data(), arg.data(), (int32_t)op.size(),
                                             out.data(), &m));
        return {out, m};
    }
    double skew(const std::string &c) const {                                   // functions.rs:1617-1640
        const auto st = moments(c, PANDRS_HIP_MOMENTS_WANT_CENTRAL);
        if (st.count < 3) return std::nan("");                                  // :1621
        const double n = (double)st.count, std_dev = std::sqrt(st.m2 / n);
        if (std_dev == 0.0) return std::nan("");                                // :1630
        const double skewness = (st.m3 / n) / ((std_dev * std_dev) * std_dev);
        return skewness * (std::sqrt(n * (n - 1.0)) / (n - 2.0));               // :1638
    }
    double kurtosis(const std::string &c) const {                               // functions.rs:1642-1665
        const auto st = moments(c, PANDRS_HIP_MOMENTS_WANT_CENTRAL);
        if (st.count < 4) return std::nan("");                                  // :1646
        const double n = (double)st.count, std_dev = std::sqrt(st.m2 / n);
        if (std_dev == 0.0) return std::nan("");                                // :1655
        const double k = (st.m4 / n) / ((std_dev * std_dev) * (std_dev * std_dev)) - 3.0;
        return ((n - 1.0) / ((n - 2.0) * (n - 3.0))) * ((n + 1.0) * k + 6.0);   // :1663
    }
    double var_column(const std::string &c, size_t ddof = 1) const {            // functions.rs:3571-3584
        const auto st = moments(c, PANDRS_HIP_MOMENTS_WANT_CENTRAL);
        if ((size_t)st.count <= ddof) return std::nan("");                      // :3575
        return st.m2 / ((double)st.count - (double)ddof);
    }
    double std_column(const std::string &c, size_t ddof = 1) const { return std::sqrt(var_column(c, ddof)); }      // :3586-3588
    double sem(const std::string &c, size_t ddof = 1) const {                   // aggregations.rs:8-23
        const auto st = moments(c, PANDRS_HIP_MOMENTS_WANT_CENTRAL);
        if ((size_t)st.count <= ddof) return std::nan("");                      // :12
        return std::sqrt(st.m2 / (double)((size_t)st.count - ddof)) / std::sqrt((double)st.count);
    }
    double mad(const std::string &c) const {                                    // aggregations.rs:26-39
        const auto st = moments(c, PANDRS_HIP_MOMENTS_WANT_CENTRAL);
        return st.count ? st.abs_dev / (double)st.count : std::nan("");
    }
    double prod(const std::string &c) const {                                   // aggregations.rs:42-51
        const auto st = moments(c, PANDRS_HIP_MOMENTS_WANT_PROD);
        return st.count ? st.prod : std::nan("");
    }
    double range(const std::string &c) const {                                  // functions.rs:4207-4219
        const auto st = moments(c, 0);
        return st.count ? st.max - st.min : std::nan("");
    }
    double abs_sum(const std::string &c) const { return moments(c, 0).abs_sum; }      // functions.rs:4221-4224
    double cv(const std::string &c) const {                                     // aggregations.rs:162-181
        const auto st = moments(c, PANDRS_HIP_MOMENTS_WANT_CENTRAL);
        if (!st.count) return std::nan("");                                     // :166
        if (std::fabs(st.mean) < std::numeric_limits<double>::epsilon()) return std::nan("");      // :173
        return std::sqrt(st.m2 / std::max((double)st.count - 1.0, 1.0)) / std::fabs(st.mean);
    }
    double geometric_mean(const std::string &c) const {                         // aggregations.rs:108-122
        const auto st = moments(c, PANDRS_HIP_MOMENTS_WANT_LOG);
        return st.count_pos ? std::exp(st.log_sum / (double)st.count_pos) : std::nan("");
    }
    double harmonic_mean(const std::string &c) const {                          // aggregations.rs:125-139
        const auto st = moments(c, PANDRS_HIP_MOMENTS_WANT_RECIP);
        return st.count_nonzero ? (double)st.count_nonzero / st.recip_sum : std::nan("");
    }
    double iqr(const std::string &c) const {                                    // aggregations.rs:142-159
        const auto r = order_stats(c, {{PANDRS_HIP_OS_AT_FRAC_N, 0.25}, {PANDRS_HIP_OS_AT_FRAC_N, 0.75}});
        return r.second < 2 ? std::nan("") : r.first[1] - r.first[0];
    }
    // percentile_value / trimmed_mean, two deviations from the reference: the column is looked up first, so a missing or non-numeric
    // column throws ColumnNotFound / Type even for an argument outside the accepted range (the reference returns NaN there before
    // it looks at the column); a NaN argument throws InvalidValue (the reference's comparisons let it through, and `NaN as usize`
    // indexes element 0 / trims nothing).
    double percentile_value(const std::string &c, double q) const {             // aggregations.rs:184-200
        numeric(c);
        if (q != q) throw Error(Error::InvalidValue, "q must not be NaN");
        if (q < 0.0 || q > 1.0) return std::nan("");                            // :185, before any device call
        return order_stats(c, {{PANDRS_HIP_OS_AT_FRAC_N1, q}}).first[0];
    }
    double trimmed_mean(const std::string &c, double trim_fraction) const {     // aggregations.rs:203-225
        numeric(c);
        if (trim_fraction != trim_fraction) throw Error(Error::InvalidValue, "trim_fraction must not be NaN");
        if (trim_fraction < 0.0 || trim_fraction >= 0.5) return std::nan("");   // :204, before any device call
        return order_stats(c, {{PANDRS_HIP_OS_TRIMMED_MEAN, trim_fraction}}).first[0];
    }
    std::map<std::string, double> describe_column(const std::string &c) const { // aggregations.rs:54-105
        const auto st = moments(c, PANDRS_HIP_MOMENTS_WANT_CENTRAL);
        const double nan = std::nan("");
        if (!st.count) return {{"count", 0.0}, {"mean", nan}, {"std", nan}, {"min", nan}, {"max", nan}};     // :60-67
        const double n = (double)st.count;
        const auto q = order_stats(c, {{PANDRS_HIP_OS_AT_FRAC_N, 0.25}, {PANDRS_HIP_OS_AT_FRAC_N, 0.5}, {PANDRS_HIP_OS_AT_FRAC_N, 0.75}}).first;
        return {{"count", n}, {"mean", st.mean}, {"std", std::sqrt(st.m2 / std::max(n - 1.0, 1.0))}, {"min", st.min}, {"max", st.max},
                {"25%", q[0]}, {"50%", q[1]}, {"75%", q[2]}};
    }
    std::vector<double> zscore(const std::string &c) const {                    // functions.rs:2284-2314
        const auto st = moments(c, PANDRS_HIP_MOMENTS_WANT_CENTRAL);
        if (st.count < 2) throw Error(Error::InvalidValue, "Need at least 2 values for z-score");              // :2288
        const double std_dev = std::sqrt(st.m2 / ((double)st.count - 1.0));
        if (std_dev == 0.0) throw Error(Error::InvalidValue, "Standard deviation is zero");                    // :2298
        return eval({c}, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_CONST, st.mean}, {PANDRS_HIP_EVAL_SUB, 0}, {PANDRS_HIP_EVAL_CONST, std_dev},
                          {PANDRS_HIP_EVAL_DIV, 0}});
    }
    // the per-frame lists: every Int64 / Float64 column in column order, PANDRS_HIP_MOMENTS_MAX_COLUMNS per call
    std::vector<std::pair<std::string, pandrs_hip_moments_stats>> moments_all(uint32_t want) const {
        std::vector<std::string> names;
        for (size_t i = 0; i < columns.size(); i++)
            if (columns[i].index() <= 1) names.push_back(column_names[i]);
        std::vector<std::pair<std::string, pandrs_hip_moments_stats>> out;
        for (size_t i = 0; i < names.size(); i += PANDRS_HIP_MOMENTS_MAX_COLUMNS) {
            const size_t k = std::min(names.size() - i, (size_t)PANDRS_HIP_MOMENTS_MAX_COLUMNS);
            std::vector<pandrs_hip_column> v;
            for (size_t j = 0; j < k; j++) v.push_back(view_of(names[i + j]));
            std::vector<pandrs_hip_moments_stats> st(k);
            detail::check(pandrs_hip_moments(detail::context(), mem_space(), v.data(), (int32_t)k, (int64_t)row_count_, want, st.data()));
            for (size_t j = 0; j < k; j++) out.emplace_back(names[i + j], st[j]);
        }
        return out;
    }
    using NamedValues = std::vector<std::pair<std::string, double>>;
    NamedValues sum_all() const {                                               // functions.rs:934-943
        NamedValues r;
        for (auto &e : moments_all(0)) r.emplace_back(e.first, e.second.sum);
        return r;
    }
    NamedValues mean_all() const {                                              // :944-957
        NamedValues r;
        for (auto &e : moments_all(0)) if (e.second.count) r.emplace_back(e.first, e.second.mean);
        return r;
    }
    NamedValues var_all() const {                                               // :975-991
        NamedValues r;
        for (auto &e : moments_all(PANDRS_HIP_MOMENTS_WANT_CENTRAL))
            if (e.second.count > 1) r.emplace_back(e.first, e.second.m2 / (double)(e.second.count - 1));
        return r;
    }
    NamedValues std_all() const {                                               // :958-974
        NamedValues r = var_all();
        for (auto &e : r) e.second = std::sqrt(e.second);
        return r;
    }
    NamedValues min_all() const {                                               // :992-1005
        NamedValues r;
        for (auto &e : moments_all(0)) if (e.second.count) r.emplace_back(e.first, e.second.min);
        return r;
    }
    NamedValues max_all() const {                                               // :1006-1022
        NamedValues r;
        for (auto &e : moments_all(0)) if (e.second.count) r.emplace_back(e.first, e.second.max);
        return r;
    }
    NamedValues product_all() const {                                           // :1583-1595
        NamedValues r;
        for (auto &e : moments_all(PANDRS_HIP_MOMENTS_WANT_PROD)) if (e.second.count) r.emplace_back(e.first, e.second.prod);
        return r;
    }
    NamedValues median_all() const {                                            // :1597-1615
        NamedValues r;
        for (size_t i = 0; i < columns.size(); i++) {
            if (columns[i].index() > 1) continue;
            const auto m = order_stats(column_names[i], {{PANDRS_HIP_OS_MEDIAN, 0.0}});
            if (m.second) r.emplace_back(column_names[i], m.first[0]);
        }
        return r;
    }
    // value_range / cut / qcut (PandasCompatExt, src/dataframe/pandas_compat/functions.rs:2270-2282, :2339-2420).  value_range:
    // (min, max) over the cells that are not NaN, from the whole-column reduction.  cut: `bins` equal-width bins over that range,
    // the last edge max + 0.001; "(lo, hi]" with two decimals for the first bin with lo <= v < hi, "NaN" for a NaN or null cell,
    // and NO entry for a row that matches no bin (the maximum once max + 0.001 == max): the vector is then shorter than the
    // column, as the reference's is.  qcut: edges at valid[min(m * i / q, m - 1)], "Q{i + 1}", "NaN", "" for a row in no bin.
    // One pandrs_hip_bin_edges call (the reference's edge list, bit for bit) and one pandrs_hip_bin call each.  InvalidValue for
    // bins == 0 / q == 0, more than PANDRS_HIP_BIN_MAX_BINS, or no valid cell; ColumnNotFound / Type before any device call.
    std::pair<double, double> value_range(const std::string &column_name) const {
        numeric(column_name);
        if (!row_count_) throw Error(Error::InvalidValue, "No valid values in column");
        const pandrs_hip_column_stats st = stats(column_name);
        if (st.min > st.max) throw Error(Error::InvalidValue, "No valid values in column");
        return {st.min, st.max};
    }
    std::vector<std::string> cut(const std::string &column_name, size_t bins) const {
        numeric(column_name);
        if (bins == 0) throw Error(Error::InvalidValue, "Number of bins must be > 0");
        std::vector<double> edges;
        std::vector<int32_t> codes;
        const size_t n_nan = bin(column_name, PANDRS_HIP_BIN_CUT, bins, "No valid values in column", edges, codes);
        if (codes.empty() && row_count_) return std::vector<std::string>(n_nan, "NaN");     // w is not finite: every bin is empty
        std::vector<std::string> labels(bins), out;
        out.reserve(row_count_);
        for (int32_t code : codes) {
            if (code == PANDRS_HIP_BIN_NONE) continue;
            if (code == PANDRS_HIP_BIN_NAN) { out.emplace_back("NaN"); continue; }
            if (labels[(size_t)code].empty()) {
                char buf[700];                                                              // two %.2f of any finite double
                std::snprintf(buf, sizeof buf, "(%.2f, %.2f]", edges[(size_t)code], edges[(size_t)code + 1]);
                labels[(size_t)code] = buf;
            }
            out.push_back(labels[(size_t)code]);
        }
        return out;
    }
    std::vector<std::string> qcut(const std::string &column_name, size_t q) const {
        numeric(column_name);
        if (q == 0) throw Error(Error::InvalidValue, "Number of quantiles must be > 0");
        std::vector<double> edges;
        std::vector<int32_t> codes;
        bin(column_name, PANDRS_HIP_BIN_QCUT, q, "No valid values", edges, codes);
        std::vector<std::string> out(row_count_);
        for (size_t r = 0; r < row_count_; r++)
            if (codes[r] == PANDRS_HIP_BIN_NAN) out[r] = "NaN";
            else if (codes[r] >= 0) out[r] = "Q" + std::to_string(codes[r] + 1);
        return out;
    }
    // value_counts / unique / nunique / mode / is_unique (PandasCompatExt, src/dataframe/pandas_compat/functions.rs:343-384,
    // :775-788, :1709-1753, :4120-4139, :4226-4259): one pandrs_hip_distinct call each (the distinct values and their exact counts,
    // ordered on the device), the list of distinct values assembled on the host.  A missing cell behaves as NaN for a numeric
    // column (one (NaN, nan_count + null_count) entry, as in cut and fillna) and as "" otherwise.  Deviations (pandrs_hip.h): all
    // NaN payloads are one entry; -0.0 comes before 0.0 where the reference's order is HashMap order; Int64 cells are counted as
    // integers; mode_with_count returns the SMALLEST of the numbers that share the largest count (the reference: an arbitrary one).
    // ColumnNotFound / Type before any device call.
    std::vector<std::pair<std::string, size_t>> value_counts(const std::string &column_name) const {
        const Column &c = column(column_name);
        bool merged = false;
        auto entries = string_entries(column_name, PANDRS_HIP_DISTINCT_BY_COUNT, &merged);
        if (merged || c.index() != 2)      // a String column arrives ordered (count descending, then its strings through the rank table)
            std::stable_sort(entries.begin(), entries.end(), [](const auto &a, const auto &b) { return a.second != b.second ? a.second > b.second : a.first < b.first; });
        return entries;
    }
    std::vector<std::pair<double, size_t>> value_counts_numeric(const std::string &column_name) const {
        numeric(column_name);
        const DistinctList d = distinct(column_name, PANDRS_HIP_DISTINCT_BY_COUNT);
        std::vector<std::pair<double, size_t>> out;
        const size_t missing = (size_t)(d.info.nan_count + d.info.null_count);
        bool placed = missing == 0;
        for (size_t i = 0; i < d.values.size(); i++) {
            if (d.flags[i]) continue;
            if (!placed && (size_t)d.counts[i] < missing) { out.emplace_back(std::nan(""), missing); placed = true; }
            out.emplace_back(cell_f64(column_name, d.values[i]), (size_t)d.counts[i]);
        }
        if (!placed) out.emplace_back(std::nan(""), missing);
        return out;
    }
    std::vector<std::string> unique(const std::string &column_name) const {
        std::vector<std::string> out;
        for (auto &e : string_entries(column_name, PANDRS_HIP_DISTINCT_BY_VALUE, nullptr)) out.push_back(e.first);
        std::sort(out.begin(), out.end());
        return out;
    }
    std::vector<double> unique_numeric(const std::string &column_name) const {
        numeric(column_name);
        const DistinctList d = distinct(column_name, PANDRS_HIP_DISTINCT_BY_VALUE);
        std::vector<double> out;
        for (size_t i = 0; i < d.values.size(); i++)
            if (!d.flags[i]) out.push_back(cell_f64(column_name, d.values[i]));
        if (d.info.nan_count + d.info.null_count) out.push_back(std::nan(""));
        return out;
    }
    std::vector<std::pair<std::string, size_t>> nunique() const {
        std::vector<std::pair<std::string, size_t>> out;
        for (auto &name : column_names) out.emplace_back(name, string_entries(name, PANDRS_HIP_DISTINCT_BY_VALUE, nullptr).size());
        return out;
    }
    std::unordered_map<std::string, size_t> nunique_all() const {
        std::unordered_map<std::string, size_t> out;
        for (auto &name : column_names) out[name] = numbers_of(distinct(name, PANDRS_HIP_DISTINCT_BY_VALUE).info);
        return out;
    }
    std::vector<double> mode_numeric(const std::string &column_name) const {
        numeric(column_name);
        const DistinctList d = distinct(column_name, PANDRS_HIP_DISTINCT_BY_VALUE);
        std::vector<double> out;
        for (size_t i = 0; i < d.values.size(); i++)
            if (!d.flags[i] && d.counts[i] == d.info.max_count) out.push_back(cell_f64(column_name, d.values[i]));
        return out;
    }
    std::vector<std::string> mode_string(const std::string &column_name) const {
        if (column(column_name).index() != 2) throw Error(Error::Type, "Column '" + column_name + "' is not a string type");
        size_t top = 0;
        auto entries = string_entries(column_name, PANDRS_HIP_DISTINCT_BY_VALUE, nullptr);
        for (auto &e : entries)
            if (!e.first.empty()) top = std::max(top, e.second);
        std::vector<std::string> out;
        for (auto &e : entries)
            if (!e.first.empty() && e.second == top) out.push_back(e.first);
        std::sort(out.begin(), out.end());
        return out;
    }
    std::pair<double, size_t> mode_with_count(const std::string &column_name) const {
        numeric(column_name);
        const DistinctList d = distinct(column_name, PANDRS_HIP_DISTINCT_BY_COUNT);
        for (size_t i = 0; i < d.values.size(); i++)
            if (!d.flags[i]) return {cell_f64(column_name, d.values[i]), (size_t)d.counts[i]};      // BY_COUNT: the largest count, then the smallest value
        return {std::nan(""), 0};
    }
    bool is_unique(const std::string &column_name) const {
        const pandrs_hip_distinct_info info = distinct(column_name, PANDRS_HIP_DISTINCT_BY_VALUE).info;
        return (int64_t)numbers_of(info) == info.n_valid;
    }
    // crosstab / pivot_table / pivot / unstack (PandasCompatExt::crosstab, functions.rs:2138-2183; DataFrame::pivot_table,
    // src/pivot/mod.rs:107-250; unstack / pivot, functions.rs:2471-2527): one pandrs_hip_pivot call each, the small label x label
    // matrix put into byte-wise string order on the host.  The result: a String column named like the index column with the
    // distinct index strings ascending, and one Float64 column per distinct columns string, ascending.  A label is stringified
    // as in value_counts; a missing cell reads "NaN" (numeric) or "" (String, Boolean).  crosstab: the rows per pair, 0.0 where
    // there is none; a missing label that reads like a literal label of its column is merged with it (the counts add), for the
    // other methods that is Error::OperationFailed.  pivot_table: the engine's Sum / Mean / Min / Max / Count of the pair's rows
    // (pandrs_hip.h), a null mask on the cells no row reaches (deviation: the reference's legacy frame writes strings, "" there,
    // and its label order is HashSet order).  unstack / pivot: the value of the pair's LAST row, NaN where there is none, no
    // mask.  Before any device call: ColumnNotFound, Type (a values column that is not numeric); a columns label equal to the
    // index column's name: DuplicateColumnName.
    OptimizedDataFrame crosstab(const std::string &col1, const std::string &col2) const {
        const PivotMatrix m = pivot_matrix(col1, col2, nullptr, PANDRS_HIP_PIVOT_ROWS, "crosstab");
        OptimizedDataFrame out;
        out.add_column(col1, StringColumn(m.index));
        for (size_t j = 0; j < m.columns.size(); j++) {
            std::vector<double> v(m.index.size());
            for (size_t i = 0; i < v.size(); i++) v[i] = (double)m.rows[j * m.index.size() + i];
            out.add_column(m.columns[j], Float64Column(std::move(v)));
        }
        return out;
    }
    OptimizedDataFrame pivot_table(const std::string &index, const std::string &columns, const std::string &values, AggFunction aggfunc) const {
        static const int32_t ops[] = {PANDRS_HIP_PIVOT_SUM, PANDRS_HIP_PIVOT_MEAN, PANDRS_HIP_PIVOT_MIN, PANDRS_HIP_PIVOT_MAX, PANDRS_HIP_PIVOT_COUNT};
        const PivotMatrix m = pivot_matrix(index, columns, &values, ops[(int)aggfunc], "pivot_table");
        OptimizedDataFrame out;
        out.add_column(index, StringColumn(m.index));
        for (size_t j = 0; j < m.columns.size(); j++) {
            const size_t R = m.index.size();
            std::vector<double> v(m.cells.begin() + j * R, m.cells.begin() + (j + 1) * R);
            std::vector<bool> nulls(R);
            bool any = false;
            for (size_t i = 0; i < R; i++) { nulls[i] = m.rows[j * R + i] == 0; any = any || nulls[i]; }
            out.add_column(m.columns[j], any ? Float64Column::with_nulls(std::move(v), nulls) : Float64Column(std::move(v)));
        }
        return out;
    }
    OptimizedDataFrame unstack(const std::string &index_col, const std::string &columns_col, const std::string &values_col) const {
        const PivotMatrix m = pivot_matrix(index_col, columns_col, &values_col, PANDRS_HIP_PIVOT_LAST, "unstack");
        OptimizedDataFrame out;
        out.add_column(index_col, StringColumn(m.index));
        for (size_t j = 0; j < m.columns.size(); j++) {
            const size_t R = m.index.size();
            out.add_column(m.columns[j], Float64Column(std::vector<double>(m.cells.begin() + j * R, m.cells.begin() + (j + 1) * R)));
        }
        return out;
    }
    OptimizedDataFrame pivot(const std::string &index, const std::string &columns, const std::string &values) const {
        return unstack(index, columns, values);                      // functions.rs:2524-2527
    }
    // cumsum / cumprod / cummax / cummin / cumcount / shift / diff / pct_change (PandasCompatExt,
    // src/dataframe/pandas_compat/functions.rs:280-342, :514-541, :2081-2094): the reference's vectors from one
    // pandrs_hip_cumulative or pandrs_hip_lag call.  Errors before any device call: ColumnNotFound, Type (a String or Boolean
    // column); an empty column gives an empty vector.  Deviations (pandrs_hip.h): a row under a null bit is skipped and answers
    // NaN (shift: nullopt; cumcount: the running count); a parallel cumsum is within 2 gamma_k sum|x| of the sequential one.
    std::vector<double> cumsum(const std::string &column_name) const { return cumulative<double>(column_name, PANDRS_HIP_CUM_SUM); }
    std::vector<double> cumprod(const std::string &column_name) const { return cumulative<double>(column_name, PANDRS_HIP_CUM_PROD); }
    std::vector<double> cummax(const std::string &column_name) const { return cumulative<double>(column_name, PANDRS_HIP_CUM_MAX); }
    std::vector<double> cummin(const std::string &column_name) const { return cumulative<double>(column_name, PANDRS_HIP_CUM_MIN); }
    std::vector<size_t> cumcount(const std::string &column_name) const {
        const std::vector<int64_t> c = cumulative<int64_t>(column_name, PANDRS_HIP_CUM_COUNT);
        return std::vector<size_t>(c.begin(), c.end());
    }
    std::vector<std::optional<double>> shift(const std::string &column_name, int32_t periods) const {
        std::vector<uint8_t> mask;
        const std::vector<double> v = lag(column_name, PANDRS_HIP_LAG_SHIFT, periods, &mask);
        std::vector<std::optional<double>> out(v.size());
        for (size_t i = 0; i < v.size(); i++)
            if (!detail::bit_at(mask, i)) out[i] = v[i];
        return out;
    }
    std::vector<double> diff(const std::string &column_name, size_t periods) const { return lag(column_name, PANDRS_HIP_LAG_DIFF, (int64_t)std::min(periods, row_count_), nullptr); }
    std::vector<double> pct_change(const std::string &column_name, size_t periods) const { return lag(column_name, PANDRS_HIP_LAG_PCT_CHANGE, (int64_t)std::min(periods, row_count_), nullptr); }
    // ---- derived columns (PandasCompatExt: functions.rs:237, :1079-1139, :2316-2337, :2819-2960, :3846-4118; helpers/math_ops.rs) ----
    // One postfix program over up to eight columns, evaluated per row in ONE pandrs_hip_eval call (pandrs_hip.h): every operation
    // is the reference's Rust expression rounded on its own; an Int64 cell loads `as f64`, a cell under a null bit as NaN (a
    // Boolean one as false).  eval: `names` are the columns COL 0, 1, ... stand for; a value program -> its cells (and the null
    // bitmap when `mask` is given: a bit where the result is NaN and a named cell of the row was null); eval_mask: a boolean
    // program -> the reference's Vec<bool>.  Errors before any device call: ColumnNotFound, Type (a String column), InvalidValue
    // (a type or limit error of the program, from pandrs_hip_eval_check, which needs no device).
    struct EvalOp { int32_t op; double arg; };
    std::vector<double> eval(const std::vector<std::string> &names, const std::vector<EvalOp> &program, std::vector<uint8_t> *mask = nullptr) const {
        if (eval_bind(names, program)) throw Error(Error::InvalidValue, "the program is a condition; eval takes a value program");
        return eval_values(eval_views(names), mem_space(), program, mask);
    }
    std::vector<bool> eval_mask(const std::vector<std::string> &names, const std::vector<EvalOp> &program) const {
        if (!eval_bind(names, program)) throw Error(Error::InvalidValue, "the program is a value; eval_mask takes a condition");
        std::vector<uint8_t> bits((row_count_ + 7) / 8);
        if (row_count_) {
            const std::vector<pandrs_hip_column> v = eval_views(names);
            std::vector<int32_t> ops;
            std::vector<double> args;
            for (const EvalOp &o : program) { ops.push_back(o.op); args.push_back(o.arg); }
            detail::check(pandrs_hip_eval(detail::context(), mem_space(), v.data(), (int32_t)v.size(), (int64_t)row_count_, ops.data(), args.data(),
                                          (int32_t)ops.size(), PANDRS_HIP_MEM_HOST, bits.data(), nullptr, nullptr));
        }
        return unpack(bits, row_count_);
    }
    // add_scalar / sub_scalar / mul_scalar / div_scalar / sqrt (functions.rs:2819-2840): the column replaced in position (Float64)
    OptimizedDataFrame add_scalar(const std::string &c, double v) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_CONST, v}, {PANDRS_HIP_EVAL_ADD, 0}}); }
    OptimizedDataFrame sub_scalar(const std::string &c, double v) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_CONST, v}, {PANDRS_HIP_EVAL_SUB, 0}}); }
    OptimizedDataFrame mul_scalar(const std::string &c, double v) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_CONST, v}, {PANDRS_HIP_EVAL_MUL, 0}}); }
    OptimizedDataFrame div_scalar(const std::string &c, double v) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_CONST, v}, {PANDRS_HIP_EVAL_DIV, 0}}); }
    OptimizedDataFrame sqrt(const std::string &c) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_SQRT, 0}}); }
    // col_add .. col_div (:2851-2960), add_columns .. div_columns (:3890-3984), coalesce (:3846-3868: v1.is_nan() ? v2 : v1): the
    // result appended as `result_name`; a name the frame already has is DuplicateColumnName (DataFrame::add_column, base.rs:143-145)
    OptimizedDataFrame col_add(const std::string &a, const std::string &b, const std::string &r) const { return zip_columns(a, b, r, PANDRS_HIP_EVAL_ADD); }
    OptimizedDataFrame col_sub(const std::string &a, const std::string &b, const std::string &r) const { return zip_columns(a, b, r, PANDRS_HIP_EVAL_SUB); }
    OptimizedDataFrame col_mul(const std::string &a, const std::string &b, const std::string &r) const { return zip_columns(a, b, r, PANDRS_HIP_EVAL_MUL); }
    OptimizedDataFrame col_div(const std::string &a, const std::string &b, const std::string &r) const { return zip_columns(a, b, r, PANDRS_HIP_EVAL_DIV); }
    OptimizedDataFrame add_columns(const std::string &a, const std::string &b, const std::string &r) const { return zip_columns(a, b, r, PANDRS_HIP_EVAL_ADD); }
    OptimizedDataFrame sub_columns(const std::string &a, const std::string &b, const std::string &r) const { return zip_columns(a, b, r, PANDRS_HIP_EVAL_SUB); }
    OptimizedDataFrame mul_columns(const std::string &a, const std::string &b, const std::string &r) const { return zip_columns(a, b, r, PANDRS_HIP_EVAL_MUL); }
    OptimizedDataFrame div_columns(const std::string &a, const std::string &b, const std::string &r) const { return zip_columns(a, b, r, PANDRS_HIP_EVAL_DIV); }
    OptimizedDataFrame coalesce(const std::string &a, const std::string &b, const std::string &r) const { return zip_columns(a, b, r, PANDRS_HIP_EVAL_SELECT); }
    // abs / abs_column, round / round_column ((x * f).round() / f, f = 10f64.powi(decimals) computed on the host as powi does), neg,
    // floor, ceil, trunc, fract, reciprocal, mod_column (fmod), floordiv (helpers/math_ops.rs:29-101): the column replaced
    OptimizedDataFrame abs(const std::string &c) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_ABS, 0}}); }
    OptimizedDataFrame abs_column(const std::string &c) const { return abs(c); }
    OptimizedDataFrame round(const std::string &c, int32_t decimals) const {
        double f = 1.0;
        for (int32_t k = 0; k < (decimals < 0 ? -decimals : decimals); k++) f *= 10.0;         // exact up to 10^22
        if (decimals < 0) f = 1.0 / f;
        return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_CONST, f}, {PANDRS_HIP_EVAL_MUL, 0}, {PANDRS_HIP_EVAL_ROUND, 0}, {PANDRS_HIP_EVAL_CONST, f}, {PANDRS_HIP_EVAL_DIV, 0}});
    }
    OptimizedDataFrame round_column(const std::string &c, int32_t decimals) const { return round(c, decimals); }
    OptimizedDataFrame neg(const std::string &c) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_NEG, 0}}); }
    OptimizedDataFrame floor(const std::string &c) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_FLOOR, 0}}); }
    OptimizedDataFrame ceil(const std::string &c) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_CEIL, 0}}); }
    OptimizedDataFrame trunc(const std::string &c) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_TRUNC, 0}}); }
    OptimizedDataFrame fract(const std::string &c) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_FRACT, 0}}); }
    OptimizedDataFrame reciprocal(const std::string &c) const { return map_column(c, {{PANDRS_HIP_EVAL_CONST, 1.0}, {PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_DIV, 0}}); }
    OptimizedDataFrame mod_column(const std::string &c, double d) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_CONST, d}, {PANDRS_HIP_EVAL_REM, 0}}); }
    OptimizedDataFrame floordiv(const std::string &c, double d) const { return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_CONST, d}, {PANDRS_HIP_EVAL_DIV, 0}, {PANDRS_HIP_EVAL_FLOOR, 0}}); }
    // clip (functions.rs:237-252), clip_lower (:3787), clip_upper (:3807): x.max(lower).min(upper); through f64::max / f64::min a NaN
    // cell clips TO THE BOUND.  The column is replaced (the reference's clip fails on its own add_column of the existing name).
    OptimizedDataFrame clip(const std::string &c, std::optional<double> lower, std::optional<double> upper) const {
        std::vector<EvalOp> p{{PANDRS_HIP_EVAL_COL, 0}};
        if (lower) { p.push_back({PANDRS_HIP_EVAL_CONST, *lower}); p.push_back({PANDRS_HIP_EVAL_MAX, 0}); }
        if (upper) { p.push_back({PANDRS_HIP_EVAL_CONST, *upper}); p.push_back({PANDRS_HIP_EVAL_MIN, 0}); }
        return map_column(c, p);
    }
    OptimizedDataFrame clip_lower(const std::string &c, double min) const { return clip(c, min, std::nullopt); }
    OptimizedDataFrame clip_upper(const std::string &c, double max) const { return clip(c, std::nullopt, max); }
    // where_cond (cond ? x : other) and mask (cond ? other : x), functions.rs:1079-1139; a condition of the wrong length: InvalidValue
    OptimizedDataFrame where_cond(const std::string &c, const std::vector<bool> &condition, double other) const { return where_impl(c, condition, other, true); }
    OptimizedDataFrame mask(const std::string &c, const std::vector<bool> &condition, double other) const { return where_impl(c, condition, other, false); }
    // fillna_zero (:4097-4118: x.is_nan() ? 0.0 : x) and replace_inf (:4026-4049: x.is_infinite() ? replacement : x)
    OptimizedDataFrame fillna_zero(const std::string &c) const {
        return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_ISNAN, 0}, {PANDRS_HIP_EVAL_CONST, 0.0}, {PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_SELECT, 0}});
    }
    OptimizedDataFrame replace_inf(const std::string &c, double replacement) const {
        return map_column(c, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_ISINF, 0}, {PANDRS_HIP_EVAL_CONST, replacement}, {PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_SELECT, 0}});
    }
    // sign (functions.rs:3998-4014): 1 / -1 / 0 per row, 0 for NaN and both zeros
    std::vector<int32_t> sign(const std::string &c) const {
        numeric(c);
        const std::vector<double> v = eval({c}, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_SIGN, 0}});
        return std::vector<int32_t>(v.begin(), v.end());
    }
    // normalize (functions.rs:2316-2337): (x - min) / (max - min), min / max over the cells that are not NaN from the whole-column
    // reduction; InvalidValue where the reference raises it (no valid value, a range of zero)
    std::vector<double> normalize(const std::string &c) const {
        numeric(c);
        if (!row_count_) throw Error(Error::InvalidValue, "No valid values in column");
        const pandrs_hip_column_stats st = stats(c);
        if (st.min > st.max) throw Error(Error::InvalidValue, "No valid values in column");
        const double range = st.max - st.min;
        if (range == 0.0) throw Error(Error::InvalidValue, "Range is zero, cannot normalize");
        return eval({c}, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_CONST, st.min}, {PANDRS_HIP_EVAL_SUB, 0}, {PANDRS_HIP_EVAL_CONST, range}, {PANDRS_HIP_EVAL_DIV, 0}});
    }
    // ffill / bfill / fillna_method / interpolate / fillna (PandasCompatExt, src/dataframe/pandas_compat/functions.rs:789-918,
    // :3626-3683): a NEW frame from one pandrs_hip_fill call, the named column replaced (same name, same position; Float64
    // after interpolate; a null mask only when rows are still missing), the other columns copied as they are.  A cell is
    // missing when its null bit is set or, for Float64, when it is NaN.  Errors before any device call: ColumnNotFound, Type
    // (a String or Boolean column), InvalidValue (an unknown fill method; a fillna value an Int64 column cannot hold).
    // Deviations (pandrs_hip.h): the reference casts every numeric column to f64 and knows no null mask here; Int64 stays
    // Int64 under ffill / bfill / fillna.
    OptimizedDataFrame ffill(const std::string &column_name) const { return fill(column_name, PANDRS_HIP_FILL_FFILL, 0); }
    OptimizedDataFrame bfill(const std::string &column_name) const { return fill(column_name, PANDRS_HIP_FILL_BFILL, 0); }
    OptimizedDataFrame interpolate(const std::string &column_name) const { return fill(column_name, PANDRS_HIP_FILL_LINEAR, 0); }
    OptimizedDataFrame fillna_method(const std::string &column_name, const std::string &method) const {
        (void)column(column_name);
        if (method == "ffill" || method == "forward") return ffill(column_name);
        if (method == "bfill" || method == "backward") return bfill(column_name);
        throw Error(Error::InvalidValue, "Invalid fill method: '" + method + "'. Use 'ffill' or 'bfill'.");     // functions.rs:846-851
    }
    OptimizedDataFrame fillna(const std::string &column_name, double value) const {
        const Column &c = column(column_name);
        uint64_t bits = 0;
        if (c.index() == 0) {
            if (!(value >= -9223372036854775808.0 && value < 9223372036854775808.0) || value != std::floor(value))
                throw Error(Error::InvalidValue, "an Int64 column is filled with an integer that fits int64");
            bits = (uint64_t)(int64_t)value;
        } else {
            std::memcpy(&bits, &value, 8);
        }
        return fill(column_name, PANDRS_HIP_FILL_VALUE, bits);
    }
    // ---- row masks (PandasCompatExt: helpers/comparison_ops.rs:7-46, functions.rs:141-158, :253-257, :4141-4161) ----
    // gt / ge / lt / le / eq_value / ne_value / between / is_between / isna / notna / is_finite / is_infinite: the reference's
    // Vec<bool>, from one pandrs_hip_predicate call.  Every compare happens in f64 (an Int64 cell as `v as f64`); a cell under a
    // null bit behaves as NaN (pandrs_hip.h).  Errors before any device call: ColumnNotFound, Type (a String or Boolean column).
    std::vector<bool> gt(const std::string &column_name, double value) const { return predicate(column_name, PANDRS_HIP_PRED_GT, value); }
    std::vector<bool> ge(const std::string &column_name, double value) const { return predicate(column_name, PANDRS_HIP_PRED_GE, value); }
    std::vector<bool> lt(const std::string &column_name, double value) const { return predicate(column_name, PANDRS_HIP_PRED_LT, value); }
    std::vector<bool> le(const std::string &column_name, double value) const { return predicate(column_name, PANDRS_HIP_PRED_LE, value); }
    std::vector<bool> eq_value(const std::string &column_name, double value) const { return predicate(column_name, PANDRS_HIP_PRED_EQ, value); }
    std::vector<bool> ne_value(const std::string &column_name, double value) const { return predicate(column_name, PANDRS_HIP_PRED_NE, value); }
    std::vector<bool> between(const std::string &column_name, double lower, double upper) const {
        return predicate(column_name, PANDRS_HIP_PRED_BETWEEN, lower, upper);
    }
    std::vector<bool> is_between(const std::string &column_name, double lower, double upper, bool inclusive = true) const {
        return predicate(column_name, inclusive ? PANDRS_HIP_PRED_BETWEEN : PANDRS_HIP_PRED_BETWEEN_EXCLUSIVE, lower, upper);
    }
    std::vector<bool> isna(const std::string &column_name) const { return predicate(column_name, PANDRS_HIP_PRED_ISNA); }
    std::vector<bool> notna(const std::string &column_name) const { return predicate(column_name, PANDRS_HIP_PRED_NOTNA); }
    std::vector<bool> is_finite(const std::string &column_name) const { return predicate(column_name, PANDRS_HIP_PRED_IS_FINITE); }
    std::vector<bool> is_infinite(const std::string &column_name) const { return predicate(column_name, PANDRS_HIP_PRED_IS_INFINITE); }
    // count_na / has_nulls / count_value (functions.rs:3837-3840, :4187-4190, :4089-4095): the count-only form, no mask is written
    size_t count_na(const std::string &column_name) const { return predicate_count(column_name, PANDRS_HIP_PRED_ISNA, 0.0); }
    bool has_nulls(const std::string &column_name) const { return predicate_count(column_name, PANDRS_HIP_PRED_ISNA, 0.0) > 0; }
    size_t count_value(const std::string &column_name, double value) const { return predicate_count(column_name, PANDRS_HIP_PRED_EQ, value); }
    // query_gt / query_lt / query_eq / dropna (functions.rs:2776-2795, :920-929): predicate -> filter_indices -> filter_gather,
    // the frame assembled as filter assembles its own (this mirror keeps the mask in host memory, as it keeps its columns)
    OptimizedDataFrame query_gt(const std::string &column_name, double value) const { return predicate_rows(column_name, PANDRS_HIP_PRED_GT, value); }
    OptimizedDataFrame query_lt(const std::string &column_name, double value) const { return predicate_rows(column_name, PANDRS_HIP_PRED_LT, value); }
    OptimizedDataFrame query_eq(const std::string &column_name, double value) const { return predicate_rows(column_name, PANDRS_HIP_PRED_EQ, value); }
    OptimizedDataFrame dropna(const std::string &column_name) const { return predicate_rows(column_name, PANDRS_HIP_PRED_NOTNA, 0.0); }
    // isin_numeric (functions.rs:150-158): the cell's f64 bits are in the list's (-0.0 is not 0.0); a null cell never matches
    std::vector<bool> isin_numeric(const std::string &column_name, const std::vector<double> &values) const {
        const Column &c = column(column_name);
        if (c.index() > 1) throw Error(Error::Type, "Column '" + column_name + "' is not a numeric type");
        return isin_call(column_name, pandrs_hip_column{values.data(), nullptr, PANDRS_HIP_F64, 0}, (int64_t)values.size());
    }
    // isin (functions.rs:141-149) on a String column, through pool codes; a string the pool has never seen is dropped from the list
    std::vector<bool> isin(const std::string &column_name, const std::vector<std::string> &values) const {
        const Column &c = column(column_name);
        if (c.index() != 2) throw Error(Error::Type, "Column '" + column_name + "' is not a string type");
        std::vector<uint32_t> codes;
        for (auto &s : values)
            if (auto code = StringPool::global().find(s)) codes.push_back(*code);
        return isin_call(column_name, pandrs_hip_column{codes.data(), nullptr, PANDRS_HIP_U32CODE, 0}, (int64_t)codes.size());
    }
    // describe_all (stats.rs:157-171): every Int64 / Float64 column; one whose describe fails with InvalidValue is left out
    std::map<std::string, StatDescribe> describe_all() const {
        std::map<std::string, StatDescribe> results;
        for (size_t i = 0; i < columns.size(); i++) {
            if (columns[i].index() > 1) continue;
            try {
                results.emplace(column_names[i], describe(column_names[i]));
            } catch (const Error &e) {
                if (e.kind != Error::InvalidValue) throw;
            }
        }
        return results;
    }

    // sort.rs:18-143 / :146-272: the rows ordered by by[0], then by[1], ... (ascending: one flag per column, empty =
    // all ascending).  Stable, also descending; nulls last in both directions; strings in byte-wise order; NaN after
    // every number and before nulls (pandrs_hip.h).  The frame is select_rows_by_indices_impl's (select.rs:172-226):
    // nulls become 0 / 0.0 / "" / false, no null masks, no columns when there are no rows.  The columns keep this
    // frame's order (the reference emits them in HashMap order, which is unspecified).
    OptimizedDataFrame sort_by(const std::string &by, bool ascending) const { return sort_by_columns({by}, {ascending}); }
    OptimizedDataFrame sort_by_columns(const std::vector<std::string> &by, const std::vector<bool> &ascending = {}) const {
        if (by.empty()) throw Error(Error::EmptyColumnList, "empty column list");
        for (auto &name : by) if (!contains_column(name)) throw Error(Error::ColumnNotFound, name);
        if (!ascending.empty() && ascending.size() != by.size())
            throw Error(Error::InconsistentArrayLengths, "Inconsistent array lengths: expected " + std::to_string(by.size()) +
                                                         ", found " + std::to_string(ascending.size()));
        OptimizedDataFrame out;
        if (row_count_ == 0) return out;
        std::vector<pandrs_hip_column> keys;
        std::vector<int32_t> asc;
        bool strings = false;
        for (size_t k = 0; k < by.size(); k++) {
            keys.push_back(view_of(by[k]));
            asc.push_back(ascending.empty() || ascending[k] ? 1 : 0);
            strings = strings || keys.back().dtype == PANDRS_HIP_U32CODE;
        }
        std::vector<uint32_t> rank = strings ? StringPool::global().rank_table() : std::vector<uint32_t>{};
        const uint32_t *rank_ptr = rank.data();
        detail::Staged staged_rank;
        if (strings && is_resident()) rank_ptr = staged_rank.upload(rank);     // one memory space per call
        std::vector<int64_t> idx(row_count_);
        detail::check(pandrs_hip_sort_indices(detail::context(), mem_space(), keys.data(), (int32_t)keys.size(), asc.data(),
                                              strings ? rank_ptr : nullptr, (int64_t)rank.size(), (int64_t)row_count_,
                                              PANDRS_HIP_MEM_HOST, idx.data()));
        for (size_t c = 0; c < columns.size(); c++) out.add_column(column_names[c], gather(columns[c], idx));
        return out;
    }

    // data_ops.rs:124-209: row gather of every column; nulls become 0 / 0.0 / "" / false
    OptimizedDataFrame filter_by_indices(const std::vector<int64_t> &indices) const {
        std::vector<int64_t> idx;
        for (int64_t i : indices) if (i >= 0 && (size_t)i < row_count_) idx.push_back(i);
        OptimizedDataFrame out;
        for (size_t c = 0; c < columns.size(); c++) out.add_column(column_names[c], gather(columns[c], idx));
        return out;
    }

    // data_ops.rs:15-34: the named columns, in the order given, null masks kept; host only
    OptimizedDataFrame select(const std::vector<std::string> &names) const {
        OptimizedDataFrame out;
        for (auto &name : names) out.add_column(name, column(name));
        return out;
    }
    // data_ops.rs:37-121 (filter_rows, row_ops.rs:26-130, is the same body): the rows whose Boolean condition is
    // Some(true), in order; nulls become 0 / 0.0 / "" / false and there are no masks; no selected row keeps every
    // column with 0 rows.  Missing column: ColumnNotFound; not Boolean: ColumnTypeMismatch (data_ops.rs:115).
    OptimizedDataFrame filter(const std::string &condition_column) const {
        const pandrs_hip_column cond = condition(condition_column);
        if (row_count_ == 0) return empty_columns();
        return compact(cond, mem_space()).first;
    }
    OptimizedDataFrame filter_rows(const std::string &condition_column) const { return filter(condition_column); }
    // parallel.rs:21-230: filter's rows; no selected row: explicitly empty typed columns (parallel.rs:73-90)
    OptimizedDataFrame par_filter(const std::string &condition_column) const {
        const pandrs_hip_column cond = condition(condition_column);
        if (row_count_ == 0) return empty_columns();
        auto r = compact(cond, mem_space());
        return r.second ? std::move(r.first) : empty_columns();
    }
    // select.rs:150-167 through select_rows_by_indices_impl (:172-226): no selected row is a frame with NO columns; a
    // mask of the wrong length is Error::Format.  The mask is packed to bits and filtered on the device.  The columns
    // keep this frame's order (the reference emits them in HashMap order, which is unspecified).
    OptimizedDataFrame select_by_mask(const std::vector<bool> &mask) const {
        if (mask.size() != row_count_)
            throw Error(Error::Format, "Mask length (" + std::to_string(mask.size()) + ") does not match DataFrame row count (" +
                                       std::to_string(row_count_) + ")");
        if (row_count_ == 0 || columns.empty()) return OptimizedDataFrame();
        const BooleanColumn bits(mask);
        auto r = compact(pandrs_hip_column{bits.bits.data(), nullptr, PANDRS_HIP_BOOLBITS, 0}, PANDRS_HIP_MEM_HOST);
        return r.second ? std::move(r.first) : OptimizedDataFrame();
    }

    // ---- window statistics (dataframe/window.rs:13-160 over series/window.rs) ----
    // rolling (:45-79): row i's window [max(0, i+1-w), i+1), or centred start = i >= w/2 ? i - w/2 : 0,
    // end = min(start+w, n); operation sum / mean / var / std (ddof) / min / max / count, any case; min_periods < 0 =
    // window_size.  The result: every column, then a Float64Column new_column_name or "{column}_{operation}" (NaN =
    // None).  Errors before any device call: ColumnNotFound, ColumnTypeMismatch (not Int64 / Float64), InvalidValue
    // (window_size 0, an unknown operation), DuplicateColumnName.
    OptimizedDataFrame rolling(size_t window_size, const std::string &column_name, const std::string &operation,
                               const std::string &new_column_name = "", int64_t min_periods = -1, bool center = false,
                               int64_t ddof = 1) const {
        window_column(column_name);
        if (window_size == 0) throw Error(Error::InvalidValue, "Window size must be greater than 0");
        pandrs_hip_window_spec sp{PANDRS_HIP_WINDOW_KIND_ROLLING, window_op("rolling", operation, false), (int64_t)window_size,
                                  min_periods, center ? 1 : 0, 0, ddof, 0.0};
        return with_window(column_name, operation, new_column_name, sp);
    }
    // expanding (:82-119): row i's window [0, i+1), min_periods as given
    OptimizedDataFrame expanding(size_t min_periods, const std::string &column_name, const std::string &operation,
                                 const std::string &new_column_name = "", int64_t ddof = 1) const {
        window_column(column_name);
        pandrs_hip_window_spec sp{PANDRS_HIP_WINDOW_KIND_EXPANDING, window_op("expanding", operation, false), 0,
                                  (int64_t)min_periods, 0, 0, ddof, 0.0};
        return with_window(column_name, operation, new_column_name, sp);
    }
    // ewm (:122-160): alpha = 2/(span+1) when span > 0 is given, else alpha (validated to (0, 1], series/window.rs:567-573),
    // else 1 - exp(-ln2/halflife) (get_alpha, :608); operation mean / std / var (var = the std output squared)
    OptimizedDataFrame ewm(const std::string &column_name, const std::string &operation, const size_t *span,
                           const double *alpha, const std::string &new_column_name = "", const double *halflife = nullptr) const {
        window_column(column_name);
        double a;
        if (span) a = 2.0 / ((double)*span + 1.0);
        else if (alpha) {
            if (!(*alpha > 0.0 && *alpha <= 1.0)) throw Error(Error::InvalidValue, "Alpha must be between 0 and 1");
            a = *alpha;
        } else if (halflife) a = 1.0 - std::exp(-0.69314718055994530942 / *halflife);
        else throw Error(Error::InvalidValue, "Must specify either span or alpha for EWM");
        if (!std::isfinite(a)) throw Error(Error::InvalidValue, "EWM alpha is not finite");
        pandrs_hip_window_spec sp{PANDRS_HIP_WINDOW_KIND_EWM, window_op("EWM", operation, true), 0, 0, 0, 0, 0, a};
        return with_window(column_name, operation, new_column_name, sp);
    }

    // ---- window order statistics (helpers/window_ops.rs:206-240; dataframe/enhanced_window.rs) ----
    // PandasCompatExt::rolling_median (pandas_compat/functions.rs:2055): the median of the trailing window's non-null,
    // non-NaN cells; NaN where fewer than min_periods (< 0: window) of them, or none, are there; window 0 acts as 1.
    std::vector<double> rolling_median(const std::string &column_name, size_t window, int64_t min_periods = -1) const {
        window_column(column_name);
        std::vector<double> out(row_count_);
        if (row_count_) {
            const pandrs_hip_window_quantile_spec sp{PANDRS_HIP_WINDOW_KIND_ROLLING, 1, (int64_t)std::max<size_t>(window, 1),
                                                     min_periods < 0 ? (int64_t)window : min_periods, 0, 1, 0.5};
            const pandrs_hip_column v = view_of(column_name);
            detail::check(pandrs_hip_window_quantile(detail::context(), mem_space(), &v, (int64_t)row_count_, &sp, PANDRS_HIP_MEM_HOST, out.data()));
        }
        return out;
    }
    // DataFrameWindowExt::apply_rolling / apply_expanding (enhanced_window.rs:204-216): the operations of a configuration
    inline DataFrameRollingOps apply_rolling(const DataFrameRolling &config) const;
    inline DataFrameExpandingOps apply_expanding(const DataFrameExpanding &config) const;
    // The builder's operations (enhanced_window.rs:317-424): every column of this frame, then a Float64Column
    // "{column}_{operation}" per target: the given columns, else every Int64 / Float64 column.  ws: a pandrs_hip_window
    // statistic; qs: a median / quantile.  Every error before any device call.
    OptimizedDataFrame window_columns(const std::vector<std::string> *given, const std::string &operation, const pandrs_hip_window_spec *ws,
                                      const pandrs_hip_window_quantile_spec *qs) const {
        std::vector<std::string> targets;
        if (given) {
            for (const auto &name : *given) column(name);                                  // ColumnNotFound (:414-418)
            targets = *given;
        } else {
            for (size_t c = 0; c < columns.size(); c++)
                if (columns[c].index() <= 1) targets.push_back(column_names[c]);
        }
        std::vector<std::string> names = column_names;
        for (const auto &t : targets) {
            window_column(t);
            if ((ws ? ws->kind : qs->kind) == PANDRS_HIP_WINDOW_KIND_ROLLING && (ws ? ws->window : qs->window) < 1)
                throw Error(Error::InvalidValue, "Window size must be greater than 0");      // series/window.rs:112-117
            if (qs && !qs->median && !(qs->q >= 0.0 && qs->q <= 1.0))
                throw Error(Error::InvalidValue, "Quantile must be between 0 and 1");        // series/window.rs:318-322
            const std::string name = t + "_" + operation;
            if (std::find(names.begin(), names.end(), name) != names.end()) throw Error(Error::DuplicateColumnName, "Duplicate column name: " + name);
            names.push_back(name);
        }
        OptimizedDataFrame result;
        for (size_t c = 0; c < columns.size(); c++) result.add_column(column_names[c], columns[c]);
        for (const auto &t : targets) {
            Float64Column out;
            out.data.resize(row_count_);
            if (row_count_) {
                const pandrs_hip_column v = view_of(t);
                detail::check(ws ? pandrs_hip_window(detail::context(), mem_space(), &v, (int64_t)row_count_, ws, PANDRS_HIP_MEM_HOST, out.data.data())
                                 : pandrs_hip_window_quantile(detail::context(), mem_space(), &v, (int64_t)row_count_, qs, PANDRS_HIP_MEM_HOST,
                                                              out.data.data()));
            }
            result.add_column(t + "_" + operation, std::move(out));
        }
        return result;
    }

private:
    size_t row_count_ = 0;
    std::shared_ptr<detail::ResidentSet> resident_;

    // one pandrs_hip_topk call (direction = pandrs_hip_topk_direction) -> the frame of those rows, in that order
    OptimizedDataFrame topk(size_t n, const std::string &column_name, int32_t direction) const {
        const Column &c = column(column_name);
        if (c.index() > 1) throw Error(Error::Type, "Column '" + column_name + "' is not a numeric type");
        OptimizedDataFrame out;
        if (row_count_ == 0 || n == 0) return out;
        const pandrs_hip_column v = view_of(column_name);
        std::vector<int64_t> idx(std::min(n, row_count_));
        int64_t count = 0, numbers = 0;
        detail::check(pandrs_hip_topk(detail::context(), mem_space(), &v, (int64_t)row_count_, (int64_t)idx.size(), direction,
                                      PANDRS_HIP_MEM_HOST, idx.data(), &count, &numbers));
        idx.resize((size_t)count);
        for (size_t i = 0; i < columns.size(); i++) out.add_column(column_names[i], gather(columns[i], idx));
        return out;
    }
    std::optional<size_t> arg_extreme(const std::string &column_name, int which) const {
        const Column &c = column(column_name);
        if (c.index() > 1) throw Error(Error::Type, "Column '" + column_name + "' is not a numeric type");
        int64_t rows[2] = {0, 0};
        int32_t found = 0;
        if (row_count_) {
            const pandrs_hip_column v = view_of(column_name);
            detail::check(pandrs_hip_arg_extreme(detail::context(), mem_space(), &v, (int64_t)row_count_, rows, &found));
        }
        if (!found) return std::nullopt;
        return (size_t)rows[which];
    }
    // one pandrs_hip_cumulative call (op = pandrs_hip_cum_op) -> its cells (T = int64_t for COUNT, double otherwise)
    template <typename T>
    std::vector<T> cumulative(const std::string &column_name, int32_t op) const {
        const Column &c = column(column_name);
        if (c.index() > 1) throw Error(Error::Type, "Column '" + column_name + "' is not a numeric type");
        std::vector<T> out(row_count_);
        if (row_count_) {
            const pandrs_hip_column v = view_of(column_name);
            detail::check(pandrs_hip_cumulative(detail::context(), mem_space(), &v, (int64_t)row_count_, op, PANDRS_HIP_MEM_HOST, out.data(), nullptr, nullptr));
        }
        return out;
    }
    // one pandrs_hip_lag call (op = pandrs_hip_lag_op) -> its cells, and the null bitmap when `mask` is given
    std::vector<double> lag(const std::string &column_name, int32_t op, int64_t periods, std::vector<uint8_t> *mask) const {
        const Column &c = column(column_name);
        if (c.index() > 1) throw Error(Error::Type, "Column '" + column_name + "' is not a numeric type");
        std::vector<double> out(row_count_);
        if (mask) mask->assign((row_count_ + 7) / 8, 0);
        if (row_count_) {
            const pandrs_hip_column v = view_of(column_name);
            detail::check(pandrs_hip_lag(detail::context(), mem_space(), &v, (int64_t)row_count_, op, periods, PANDRS_HIP_MEM_HOST, out.data(),
                                         mask ? mask->data() : nullptr, nullptr));
        }
        return out;
    }

    // ---- pandrs_hip_eval ----
    void numeric(const std::string &name) const {
        if (column(name).index() > 1) throw Error(Error::Type, "Column '" + name + "' is not a numeric type");
    }
    // the checks of a program that need no device -> whether it is a condition
    bool eval_bind(const std::vector<std::string> &names, const std::vector<EvalOp> &program) const {
        std::vector<int32_t> dtypes, ops;
        std::vector<double> args;
        for (const std::string &n : names) {
            const Column &c = column(n);
            if (c.index() == 2) throw Error(Error::Type, "Column '" + n + "' is not a numeric type");
            dtypes.push_back(c.index() == 0 ? PANDRS_HIP_I64 : c.index() == 1 ? PANDRS_HIP_F64 : PANDRS_HIP_BOOLBITS);
        }
        for (const EvalOp &o : program) { ops.push_back(o.op); args.push_back(o.arg); }
        int32_t is_mask = 0;
        if (pandrs_hip_eval_check(dtypes.data(), (int32_t)dtypes.size(), ops.data(), args.data(), (int32_t)ops.size(), &is_mask, nullptr) != PANDRS_HIP_OK)
            throw Error(Error::InvalidValue, pandrs_hip_last_error());
        return is_mask != 0;
    }
    std::vector<pandrs_hip_column> eval_views(const std::vector<std::string> &names) const {
        std::vector<pandrs_hip_column> v;
        for (const std::string &n : names) v.push_back(view_of(n));
        return v;
    }
    std::vector<double> eval_values(const std::vector<pandrs_hip_column> &v, int32_t space, const std::vector<EvalOp> &program, std::vector<uint8_t> *mask) const {
        std::vector<double> out(row_count_);
        if (mask) mask->assign((row_count_ + 7) / 8, 0);
        if (row_count_) {
            std::vector<int32_t> ops;
            std::vector<double> args;
            for (const EvalOp &o : program) { ops.push_back(o.op); args.push_back(o.arg); }
            detail::check(pandrs_hip_eval(detail::context(), space, v.data(), (int32_t)v.size(), (int64_t)row_count_, ops.data(), args.data(),
                                          (int32_t)ops.size(), PANDRS_HIP_MEM_HOST, out.data(), mask ? mask->data() : nullptr, nullptr));
        }
        return out;
    }
    OptimizedDataFrame with_replaced(const std::string &name, std::vector<double> values, std::vector<uint8_t> mask) const {
        Float64Column nc;
        nc.data = std::move(values);
        if (std::any_of(mask.begin(), mask.end(), [](uint8_t b) { return b != 0; })) nc.null_mask = std::move(mask);
        OptimizedDataFrame out;
        for (size_t k = 0; k < columns.size(); k++) {
            if (column_names[k] != name) out.add_column(column_names[k], columns[k]);
            else out.add_column(column_names[k], nc);
        }
        return out;
    }
    OptimizedDataFrame map_column(const std::string &name, const std::vector<EvalOp> &program) const {
        numeric(name);
        std::vector<uint8_t> mask;
        std::vector<double> v = eval({name}, program, &mask);
        return with_replaced(name, std::move(v), std::move(mask));
    }
    // op = ADD .. DIV: a op b; SELECT: isnan(a) ? b : a
    OptimizedDataFrame zip_columns(const std::string &a, const std::string &b, const std::string &result_name, int32_t op) const {
        numeric(a);
        numeric(b);
        if (column_indices.count(result_name)) throw Error(Error::DuplicateColumnName, result_name);
        std::vector<EvalOp> p{{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_COL, 1}, {op, 0}};
        if (op == PANDRS_HIP_EVAL_SELECT) p = {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_ISNAN, 0}, {PANDRS_HIP_EVAL_COL, 1}, {PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_SELECT, 0}};
        std::vector<uint8_t> mask;
        Float64Column nc;
        nc.data = a == b ? eval({a}, rename_second(p), &mask) : eval({a, b}, p, &mask);
        if (std::any_of(mask.begin(), mask.end(), [](uint8_t m) { return m != 0; })) nc.null_mask = std::move(mask);
        OptimizedDataFrame out;
        for (size_t k = 0; k < columns.size(); k++) out.add_column(column_names[k], columns[k]);
        out.add_column(result_name, std::move(nc));
        return out;
    }
    static std::vector<EvalOp> rename_second(std::vector<EvalOp> p) {      // col_add("a", "a", ..): one distinct column
        for (EvalOp &o : p)
            if (o.op == PANDRS_HIP_EVAL_COL) o.arg = 0;
        return p;
    }
    OptimizedDataFrame where_impl(const std::string &name, const std::vector<bool> &condition, double other, bool keep_where) const {
        numeric(name);
        if (condition.size() != row_count_) throw Error(Error::InvalidValue, "Condition length must match column length");       // functions.rs:1082-1086
        std::vector<uint8_t> bits((row_count_ + 7) / 8), mask;
        for (size_t i = 0; i < row_count_; i++)
            if (condition[i]) bits[i >> 3] |= (uint8_t)(1u << (i & 7));
        // the condition lives on the host, so this call reads the column's host copy too
        const std::vector<pandrs_hip_column> v{pandrs_hip_column{bits.data(), nullptr, PANDRS_HIP_BOOLBITS, 0}, detail::view(columns[column_indices.at(name)])};
        const std::vector<EvalOp> p = keep_where ? std::vector<EvalOp>{{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_COL, 1}, {PANDRS_HIP_EVAL_CONST, other}, {PANDRS_HIP_EVAL_SELECT, 0}}
                                                 : std::vector<EvalOp>{{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_CONST, other}, {PANDRS_HIP_EVAL_COL, 1}, {PANDRS_HIP_EVAL_SELECT, 0}};
        std::vector<double> out = eval_values(v, PANDRS_HIP_MEM_HOST, p, &mask);
        return with_replaced(name, std::move(out), std::move(mask));
    }

    // one pandrs_hip_fill call (method = pandrs_hip_fill_method) -> the frame with the named column replaced
    OptimizedDataFrame fill(const std::string &column_name, int32_t method, uint64_t fill_bits) const {
        const Column &c = column(column_name);
        if (c.index() > 1) throw Error(Error::Type, "Column '" + column_name + "' is not a numeric type");
        if (!row_count_) return *this;                      // an equal frame, no device call
        const bool out_i64 = c.index() == 0 && method != PANDRS_HIP_FILL_LINEAR;
        Int64Column oi;
        Float64Column of;
        std::vector<uint8_t> mask((row_count_ + 7) / 8);
        int64_t missing = 0;
        if (out_i64) oi.data.resize(row_count_); else of.data.resize(row_count_);
        const pandrs_hip_column v = view_of(column_name);
        detail::check(pandrs_hip_fill(detail::context(), mem_space(), &v, (int64_t)row_count_, method, fill_bits, PANDRS_HIP_MEM_HOST,
                                      out_i64 ? (void *)oi.data.data() : (void *)of.data.data(), mask.data(), &missing));
        if (missing) (out_i64 ? oi.null_mask : of.null_mask) = std::move(mask);
        OptimizedDataFrame out;
        for (size_t k = 0; k < columns.size(); k++) {
            if (column_names[k] != column_name) out.add_column(column_names[k], columns[k]);
            else if (out_i64) out.add_column(column_names[k], std::move(oi));
            else out.add_column(column_names[k], std::move(of));
        }
        return out;
    }

    // one pandrs_hip_predicate call (op = pandrs_hip_pred_op) -> the packed mask and its count
    std::vector<uint8_t> predicate_bits(const std::string &column_name, int32_t op, double a, double b, int64_t *count, bool want_bits) const {
        const Column &c = column(column_name);
        if (c.index() > 1) throw Error(Error::Type, "Column '" + column_name + "' is not a numeric type");
        std::vector<uint8_t> bits(want_bits ? (row_count_ + 7) / 8 : 0);
        *count = 0;
        if (!row_count_) return bits;
        const pandrs_hip_column v = view_of(column_name);
        detail::check(pandrs_hip_predicate(detail::context(), mem_space(), &v, (int64_t)row_count_, op, a, b, PANDRS_HIP_MEM_HOST,
                                           want_bits ? bits.data() : nullptr, count));
        return bits;
    }
    static std::vector<bool> unpack(const std::vector<uint8_t> &bits, size_t n) {
        std::vector<bool> out(n);
        for (size_t i = 0; i < n; i++) out[i] = (bits[i >> 3] >> (i & 7)) & 1;
        return out;
    }
    std::vector<bool> predicate(const std::string &column_name, int32_t op, double a = 0.0, double b = 0.0) const {
        int64_t count = 0;
        return unpack(predicate_bits(column_name, op, a, b, &count, true), row_count_);
    }
    size_t predicate_count(const std::string &column_name, int32_t op, double a) const {
        int64_t count = 0;
        predicate_bits(column_name, op, a, 0.0, &count, false);
        return (size_t)count;
    }
    OptimizedDataFrame predicate_rows(const std::string &column_name, int32_t op, double a) const {
        int64_t count = 0;
        const std::vector<uint8_t> bits = predicate_bits(column_name, op, a, 0.0, &count, true);
        if (row_count_ == 0) return empty_columns();
        return compact(pandrs_hip_column{bits.data(), nullptr, PANDRS_HIP_BOOLBITS, 0}, PANDRS_HIP_MEM_HOST).first;
    }
    std::vector<bool> isin_call(const std::string &column_name, const pandrs_hip_column &values, int64_t n_values) const {
        std::vector<uint8_t> bits((row_count_ + 7) / 8);
        if (row_count_) {
            int64_t count = 0;
            const pandrs_hip_column v = view_of(column_name);
            detail::check(pandrs_hip_isin(detail::context(), mem_space(), &v, (int64_t)row_count_, PANDRS_HIP_MEM_HOST, &values, n_values, 0,
                                          PANDRS_HIP_MEM_HOST, bits.data(), &count));
        }
        return unpack(bits, row_count_);
    }

    void window_column(const std::string &name) const {
        const Column &c = column(name);
        if (c.index() > 1)
            throw Error(Error::ColumnTypeMismatch, "Column type mismatch: column '" + name + "' expected Int64 or Float64");
    }
    static int32_t window_op(const char *kind, const std::string &operation, bool ewm) {
        std::string op = operation;
        std::transform(op.begin(), op.end(), op.begin(), [](unsigned char ch) { return (char)std::tolower(ch); });   // window.rs:54
        static const std::map<std::string, int32_t> ops = {{"sum", PANDRS_HIP_WINDOW_SUM}, {"mean", PANDRS_HIP_WINDOW_MEAN},
            {"var", PANDRS_HIP_WINDOW_VAR}, {"std", PANDRS_HIP_WINDOW_STD}, {"min", PANDRS_HIP_WINDOW_MIN},
            {"max", PANDRS_HIP_WINDOW_MAX}, {"count", PANDRS_HIP_WINDOW_COUNT}};
        auto it = ops.find(op);
        if (it == ops.end() || (ewm && it->second != PANDRS_HIP_WINDOW_MEAN && it->second != PANDRS_HIP_WINDOW_STD &&
                                it->second != PANDRS_HIP_WINDOW_VAR))
            throw Error(Error::InvalidValue, std::string("Unsupported ") + kind + " operation: " + operation);
        return it->second;
    }
    OptimizedDataFrame with_window(const std::string &column_name, const std::string &operation, const std::string &new_column_name,
                                   const pandrs_hip_window_spec &sp) const {
        const std::string name = new_column_name.empty() ? column_name + "_" + operation : new_column_name;   // window.rs:72
        if (std::find(column_names.begin(), column_names.end(), name) != column_names.end())
            throw Error(Error::DuplicateColumnName, "Duplicate column name: " + name);
        Float64Column out;
        out.data.resize(row_count_);
        if (row_count_) {
            const pandrs_hip_column v = view_of(column_name);
            detail::check(pandrs_hip_window(detail::context(), mem_space(), &v, (int64_t)row_count_, &sp, PANDRS_HIP_MEM_HOST,
                                            out.data.data()));
        }
        OptimizedDataFrame result;
        for (size_t c = 0; c < columns.size(); c++) result.add_column(column_names[c], columns[c]);
        result.add_column(name, std::move(out));
        return result;
    }
    pandrs_hip_column condition(const std::string &name) const {
        const Column &c = column(name);
        if (c.index() != 3)
            throw Error(Error::ColumnTypeMismatch, "Column type mismatch: column '" + name + "' expected Boolean");
        return view_of(name);
    }
    OptimizedDataFrame empty_columns() const {
        OptimizedDataFrame out;
        for (size_t c = 0; c < columns.size(); c++)
            out.add_column(column_names[c], std::visit([](auto &x) -> Column { return std::decay_t<decltype(x)>(); }, columns[c]));
        return out;
    }
    // one selection (pandrs_hip_filter_indices), then every column compacted through it (pandrs_hip_filter_gather); the
    // condition's memory space is its own (select_by_mask's mask is on the host while the columns may be resident)
    std::pair<OptimizedDataFrame, int64_t> compact(const pandrs_hip_column &cond, int32_t cond_space) const {
        int64_t n = 0;
        detail::check(pandrs_hip_filter_indices(detail::context(), cond_space, &cond, (int64_t)row_count_, PANDRS_HIP_MEM_HOST, nullptr, &n));
        OptimizedDataFrame out;
        for (size_t c = 0; c < columns.size(); c++) {
            const Column &src = columns[c];
            pandrs_hip_column v = view_of(column_names[c]);
            auto call = [&](uint64_t fill, void *o) {
                detail::check(pandrs_hip_filter_gather(detail::context(), mem_space(), &v, (int64_t)row_count_, fill, PANDRS_HIP_MEM_HOST, o));
            };
            switch (src.index()) {
            case 0: { Int64Column o; o.data.resize(n); call(0, o.data.data()); out.add_column(column_names[c], std::move(o)); break; }
            case 1: { Float64Column o; o.data.resize(n); call(0, o.data.data()); out.add_column(column_names[c], std::move(o)); break; }
            case 2: { StringColumn o; o.indices.resize(n); call(StringPool::global().get_or_insert(""), o.indices.data()); out.add_column(column_names[c], std::move(o)); break; }
            default: {
                std::vector<uint8_t> bytes(n);
                call(0, bytes.data());
                std::vector<bool> b(n);
                for (int64_t i = 0; i < n; i++) b[i] = bytes[i] != 0;
                out.add_column(column_names[c], BooleanColumn(b));
            }
            }
        }
        return {std::move(out), n};
    }

    // cut / qcut: the edge list (kind = pandrs_hip_bin_kind), then every row's code against it -> the NaN rows.  `codes` stays
    // empty where cut's w is not finite (e[0] is NaN then and every bin is empty, pandrs_hip.h).
    size_t bin(const std::string &name, int32_t kind, size_t k, const char *no_valid, std::vector<double> &edges, std::vector<int32_t> &codes) const {
        if (k > PANDRS_HIP_BIN_MAX_BINS) throw Error(Error::InvalidValue, "at most " + std::to_string(PANDRS_HIP_BIN_MAX_BINS) + " bins");
        if (!row_count_) throw Error(Error::InvalidValue, no_valid);
        const pandrs_hip_column v = view_of(name);
        edges.assign(k + 1, 0.0);
        int64_t valid = 0;
        detail::check(pandrs_hip_bin_edges(detail::context(), mem_space(), &v, (int64_t)row_count_, kind, (int32_t)k, edges.data(), &valid));
        if (valid == 0) throw Error(Error::InvalidValue, no_valid);
        if (edges[0] != edges[0]) return row_count_ - (size_t)valid;
        std::vector<double> look = edges;
        if (kind == PANDRS_HIP_BIN_QCUT) look[k] = edges[k] + 0.001;                        // functions.rs:2406-2407
        else if (look[k] < look[k - 1]) look[k] = look[k - 1];                              // (for the search only: no row lies between them)
        codes.assign(row_count_, 0);
        detail::check(pandrs_hip_bin(detail::context(), mem_space(), &v, (int64_t)row_count_, look.data(), (int32_t)k, PANDRS_HIP_MEM_HOST,
                                     codes.data(), nullptr));
        return row_count_ - (size_t)valid;
    }
    // the list of one pandrs_hip_distinct call; a String column is ordered by its strings (the pool's rank table)
    struct DistinctList {
        std::vector<uint64_t> values;
        std::vector<uint8_t> flags;        // 0 number, 1 the NaN entry, 2 the NULL entry
        std::vector<int64_t> counts;
        pandrs_hip_distinct_info info{};
    };
    DistinctList distinct(const std::string &name, int32_t order) const {
        const Column &c = column(name);
        DistinctList d;
        if (!row_count_) return d;
        const pandrs_hip_column v = view_of(name);
        const bool strings = c.index() == 2;
        std::vector<uint32_t> rank = strings ? StringPool::global().rank_table() : std::vector<uint32_t>{};
        const uint32_t *rank_ptr = rank.data();
        detail::Staged staged_rank;
        if (strings && is_resident()) rank_ptr = staged_rank.upload(rank);     // one memory space per call
        detail::check(pandrs_hip_distinct(detail::context(), mem_space(), &v, (int64_t)row_count_, order, strings ? rank_ptr : nullptr,
                                          (int64_t)rank.size(), &d.info));
        const size_t n = (size_t)d.info.n_entries;
        d.values.resize(n); d.flags.resize(n); d.counts.resize(n);
        detail::check(pandrs_hip_distinct_fetch(detail::context(), PANDRS_HIP_MEM_HOST, d.values.data(), d.flags.data(), d.counts.data()));
        return d;
    }
    static size_t numbers_of(const pandrs_hip_distinct_info &info) {
        return (size_t)(info.n_entries - (info.nan_count ? 1 : 0) - (info.null_count ? 1 : 0));
    }
    double cell_f64(const std::string &name, uint64_t cell) const {      // an entry of a numeric column as the reference's f64
        if (column(name).index() == 0) return (double)(int64_t)cell;
        double d;
        std::memcpy(&d, &cell, 8);
        return d;
    }
    // [(string, count)] in the device's order: the strings get_column_string_values gives; the missing cells as "NaN" (numeric)
    // or "", merged with such an entry of the column's own
    std::vector<std::pair<std::string, size_t>> string_entries(const std::string &name, int32_t order, bool *merged) const {
        const int32_t dtype = detail::col_dtype(column(name));
        const DistinctList d = distinct(name, order);
        std::vector<std::pair<std::string, size_t>> out;
        size_t missing = 0;
        for (size_t i = 0; i < d.values.size(); i++) {
            if (d.flags[i]) missing += (size_t)d.counts[i];
            else out.emplace_back(detail::key_string(dtype, d.values[i], false), (size_t)d.counts[i]);
        }
        if (merged) *merged = missing != 0;
        if (!missing) return out;
        const std::string as = dtype <= PANDRS_HIP_F64 ? "NaN" : "";
        for (auto &e : out)
            if (e.first == as) { e.second += missing; return out; }
        out.emplace_back(as, missing);
        return out;
    }
    // the result of one pandrs_hip_pivot call in byte-wise string order: index / columns strings, cells and rows column-major
    struct PivotMatrix {
        std::vector<std::string> index, columns;
        std::vector<double> cells;         // [j * index.size() + i]
        std::vector<int64_t> rows;
    };
    // the strings of one dimension's labels and, per output label in ascending order, the device labels that form it
    static std::vector<std::vector<size_t>> pivot_labels(int32_t dtype, const std::vector<uint64_t> &cells, const std::vector<uint8_t> &flags,
                                                         bool counts_add, const char *what, std::vector<std::string> *names) {
        std::map<std::string, std::vector<size_t>> groups;          // (std::string compares byte-wise)
        const std::string missing = dtype <= PANDRS_HIP_F64 ? "NaN" : "";
        for (size_t i = 0; i < cells.size(); i++) groups[flags[i] ? missing : detail::key_string(dtype, cells[i], false)].push_back(i);
        if (groups.size() != cells.size() && !counts_add)
            throw Error(Error::OperationFailed, std::string(what) + ": a missing cell of the key column reads like its label '" + missing + "'; the two cannot share a cell");
        std::vector<std::vector<size_t>> take;
        for (auto &g : groups) { names->push_back(g.first); take.push_back(g.second); }
        return take;
    }
    PivotMatrix pivot_matrix(const std::string &index, const std::string &columns, const std::string *values, int32_t op, const char *what) const {
        const Column &ic = column(index), &cc = column(columns);
        if (values) numeric(*values);
        PivotMatrix m;
        if (!row_count_) return m;
        const pandrs_hip_column iv = view_of(index), cv = view_of(columns);
        pandrs_hip_column vv{};
        if (values) vv = view_of(*values);
        const bool strings = ic.index() == 2 || cc.index() == 2;
        std::vector<uint32_t> rank = strings ? StringPool::global().rank_table() : std::vector<uint32_t>{};
        const uint32_t *rank_ptr = rank.data();
        detail::Staged staged_rank;
        if (strings && is_resident()) rank_ptr = staged_rank.upload(rank);     // one memory space per call
        pandrs_hip_pivot_info info{};
        detail::check(pandrs_hip_pivot(detail::context(), mem_space(), &iv, ic.index() == 2 ? rank_ptr : nullptr, ic.index() == 2 ? (int64_t)rank.size() : 0,
                                       &cv, cc.index() == 2 ? rank_ptr : nullptr, cc.index() == 2 ? (int64_t)rank.size() : 0, values ? &vv : nullptr,
                                       (int64_t)row_count_, op, &info));
        const size_t R = (size_t)info.n_index_labels, C = (size_t)info.n_column_labels;
        std::vector<uint64_t> il(R), cl(C);
        std::vector<uint8_t> fi(R), fc(C);
        std::vector<double> cells(R * C);
        std::vector<int64_t> rows(R * C);
        detail::check(pandrs_hip_pivot_fetch(detail::context(), PANDRS_HIP_MEM_HOST, il.data(), fi.data(), cl.data(), fc.data(), cells.data(), rows.data()));
        const bool add = op == PANDRS_HIP_PIVOT_ROWS;
        const auto itake = pivot_labels(detail::col_dtype(ic), il, fi, add, what, &m.index);
        const auto ctake = pivot_labels(detail::col_dtype(cc), cl, fc, add, what, &m.columns);
        for (auto &name : m.columns)
            if (name == index) throw Error(Error::DuplicateColumnName, index);
        const size_t Ro = itake.size(), Co = ctake.size();
        m.cells.assign(Ro * Co, 0.0);
        m.rows.assign(Ro * Co, 0);
        for (size_t j = 0; j < Co; j++)
            for (size_t i = 0; i < Ro; i++) {
                int64_t n = 0;
                for (size_t sj : ctake[j])
                    for (size_t si : itake[i]) n += rows[sj * R + si];
                m.rows[j * Ro + i] = n;
                m.cells[j * Ro + i] = add ? (double)n : cells[ctake[j][0] * R + itake[i][0]];
            }
        return m;
    }
    pandrs_hip_column_stats stats(const std::string &name) const {
        const Column &c = column(name);
        if (c.index() > 1) throw Error(Error::Type, "Column '" + name + "' is not a numeric type");      // aggregate.rs:57
        pandrs_hip_column v = view_of(name);
        pandrs_hip_column_stats st{};
        detail::check(pandrs_hip_reduce_stats(detail::context(), mem_space(), &v, (int64_t)detail::col_len(c), &st));
        return st;
    }
    pandrs_hip_column_stats non_empty(const std::string &name) const {
        auto st = stats(name);
        if (st.count == 0) throw Error(Error::Empty, "Column '" + name + "' is empty");                    // aggregate.rs:87
        return st;
    }
    // join_impl's / filter_by_indices' per-column gather on the device (join.rs:296-357, :475-552)
    static Column gather(const Column &src, const std::vector<int64_t> &idx) {
        const int64_t n = (int64_t)idx.size(), n_src = (int64_t)detail::col_len(src);
        pandrs_hip_column v = detail::view(src);
        auto call = [&](uint64_t fill, void *out) {
            detail::check(pandrs_hip_gather_column(detail::context(), PANDRS_HIP_MEM_HOST, &v, n_src, idx.data(), n, fill, out));
        };
        switch (src.index()) {
        case 0: { Int64Column o; o.data.resize(n); call(0, o.data.data()); return o; }
        case 1: { Float64Column o; o.data.resize(n); call(0, o.data.data()); return o; }
        case 2: { StringColumn o; o.indices.resize(n); call(StringPool::global().get_or_insert(""), o.indices.data()); return o; }
        default: {
            std::vector<uint8_t> bytes(n);
            call(0, bytes.data());
            std::vector<bool> b(n);
            for (int64_t i = 0; i < n; i++) b[i] = bytes[i] != 0;
            return BooleanColumn(b);
        }
        }
    }
    // join.rs:76-555
    OptimizedDataFrame join_impl(const OptimizedDataFrame &other, const std::string &left_on, const std::string &right_on, JoinType how) const {
        if (!contains_column(left_on)) throw Error(Error::ColumnNotFound, left_on);              // :84-87
        if (!other.contains_column(right_on)) throw Error(Error::ColumnNotFound, right_on);      // :89-92
        const Column &lc = column(left_on), &rc = other.column(right_on);
        const bool dev = is_resident() && other.is_resident();      // one memory space per call
        pandrs_hip_column lv = dev ? view_of(left_on) : detail::view(lc), rv = dev ? other.view_of(right_on) : detail::view(rc);
        int64_t n = 0;      // a key-type mismatch surfaces as ColumnTypeMismatch from the library (:98-104)
        detail::check(pandrs_hip_join_indices(detail::context(), dev ? PANDRS_HIP_MEM_DEVICE : PANDRS_HIP_MEM_HOST, &lv, (int64_t)detail::col_len(lc), &rv,
                                              (int64_t)detail::col_len(rc), (int32_t)how, &n));
        // the pairs stay in HBM (the context retains them); every output column is ONE gather through them and one
        // transfer of the finished column (pandrs_hip_join_gather) — not 16 bytes of indices per output row
        const int32_t space = dev ? PANDRS_HIP_MEM_DEVICE : PANDRS_HIP_MEM_HOST;
        OptimizedDataFrame result;
        if (n == 0) {       // empty result: NON-KEY columns only, suffix decided against the LEFT frame (:227-284)
            for (auto &name : column_names) if (name != left_on) result.add_column(name, gather(column(name), {}));
            for (auto &name : other.column_names)
                if (name != right_on) result.add_column(contains_column(name) ? name + "_right" : name, gather(other.column(name), {}));
            return result;
        }
        auto joined = [&](const OptimizedDataFrame &f, const std::string &name, int side, const pandrs_hip_column *key_right, int64_t n_right) -> Column {
            const Column &src = f.column(name);
            pandrs_hip_column v = dev ? f.view_of(name) : detail::view(src);
            const int64_t n_src = (int64_t)detail::col_len(src);
            auto call = [&](uint64_t fill, void *out) {
                if (key_right) detail::check(pandrs_hip_join_gather_key(detail::context(), space, &v, n_src, key_right, n_right, fill, PANDRS_HIP_MEM_HOST, out));
                else detail::check(pandrs_hip_join_gather(detail::context(), space, &v, n_src, side, fill, PANDRS_HIP_MEM_HOST, out));
            };
            switch (src.index()) {
            case 0: { Int64Column o; o.data.resize(n); call(0, o.data.data()); return o; }
            case 1: { Float64Column o; o.data.resize(n); call(0, o.data.data()); return o; }
            case 2: { StringColumn o; o.indices.resize(n); call(StringPool::global().get_or_insert(""), o.indices.data()); return o; }
            default: {
                std::vector<uint8_t> bytes(n);
                call(0, bytes.data());
                std::vector<bool> b(n);
                for (int64_t i = 0; i < n; i++) b[i] = bytes[i] != 0;
                return BooleanColumn(b);
            }
            }
        };
        for (auto &name : column_names) if (name != left_on) result.add_column(name, joined(*this, name, 0, nullptr, 0));     // :290-361
        result.add_column(left_on, joined(*this, left_on, 0, &rv, (int64_t)detail::col_len(rc)));       // key column: the left value, else the right one (:364-472)
        for (auto &name : other.column_names)                                                                       // :475-552
            if (name != right_on) result.add_column(result.contains_column(name) ? name + "_right" : name, joined(other, name, 1, nullptr, 0));
        return result;
    }
    friend class GroupBy;
};

// ---- GroupBy (group/types.rs:46-55) ------------------------------------------------------------------------
// DataFrameRollingOps / DataFrameExpandingOps (enhanced_window.rs:246-425, :427-560): median and quantile go to
// pandrs_hip_window_quantile, the others to pandrs_hip_window
class DataFrameRollingOps {
public:
    DataFrameRollingOps(const OptimizedDataFrame &df, const DataFrameRolling &config) : df_(df), cfg_(config) {}
    OptimizedDataFrame mean() const { return stat("mean", PANDRS_HIP_WINDOW_MEAN); }
    OptimizedDataFrame sum() const { return stat("sum", PANDRS_HIP_WINDOW_SUM); }
    OptimizedDataFrame std(size_t ddof) const { return stat("std", PANDRS_HIP_WINDOW_STD, (int64_t)ddof); }
    OptimizedDataFrame var(size_t ddof) const { return stat("var", PANDRS_HIP_WINDOW_VAR, (int64_t)ddof); }
    OptimizedDataFrame min() const { return stat("min", PANDRS_HIP_WINDOW_MIN); }
    OptimizedDataFrame max() const { return stat("max", PANDRS_HIP_WINDOW_MAX); }
    OptimizedDataFrame count() const { return stat("count", PANDRS_HIP_WINDOW_COUNT); }
    OptimizedDataFrame median() const { return order("median", 1, 0.5); }
    OptimizedDataFrame quantile(double q) const { return order("quantile", 0, q); }

private:
    const OptimizedDataFrame &df_;
    const DataFrameRolling &cfg_;
    const std::vector<std::string> *given() const { return cfg_.has_columns_ ? &cfg_.columns_ : nullptr; }
    OptimizedDataFrame stat(const char *name, int32_t op, int64_t ddof = 1) const {
        const pandrs_hip_window_spec sp{PANDRS_HIP_WINDOW_KIND_ROLLING, op, (int64_t)cfg_.window_size, cfg_.min_periods_ < 0 ? (int64_t)cfg_.window_size : cfg_.min_periods_, cfg_.center_ ? 1 : 0, 0, ddof, 0.0};
        return df_.window_columns(given(), name, &sp, nullptr);
    }
    OptimizedDataFrame order(const char *name, int32_t median, double q) const {
        const pandrs_hip_window_quantile_spec sp{PANDRS_HIP_WINDOW_KIND_ROLLING, median, (int64_t)cfg_.window_size, cfg_.min_periods_ < 0 ? (int64_t)cfg_.window_size : cfg_.min_periods_, cfg_.center_ ? 1 : 0, 0, q};
        return df_.window_columns(given(), name, nullptr, &sp);
    }
};
class DataFrameExpandingOps {
public:
    DataFrameExpandingOps(const OptimizedDataFrame &df, const DataFrameExpanding &config) : df_(df), cfg_(config) {}
    OptimizedDataFrame mean() const { return stat("mean", PANDRS_HIP_WINDOW_MEAN); }
    OptimizedDataFrame sum() const { return stat("sum", PANDRS_HIP_WINDOW_SUM); }
    OptimizedDataFrame std(size_t ddof) const { return stat("std", PANDRS_HIP_WINDOW_STD, (int64_t)ddof); }
    OptimizedDataFrame var(size_t ddof) const { return stat("var", PANDRS_HIP_WINDOW_VAR, (int64_t)ddof); }
    OptimizedDataFrame min() const { return stat("min", PANDRS_HIP_WINDOW_MIN); }
    OptimizedDataFrame max() const { return stat("max", PANDRS_HIP_WINDOW_MAX); }
    OptimizedDataFrame count() const { return stat("count", PANDRS_HIP_WINDOW_COUNT); }
    OptimizedDataFrame median() const { return order("median", 1, 0.5); }
    OptimizedDataFrame quantile(double q) const { return order("quantile", 0, q); }

private:
    const OptimizedDataFrame &df_;
    const DataFrameExpanding &cfg_;
    const std::vector<std::string> *given() const { return cfg_.has_columns_ ? &cfg_.columns_ : nullptr; }
    OptimizedDataFrame stat(const char *name, int32_t op, int64_t ddof = 1) const {
        const pandrs_hip_window_spec sp{PANDRS_HIP_WINDOW_KIND_EXPANDING, op, 0, (int64_t)cfg_.min_periods, 0, 0, ddof, 0.0};
        return df_.window_columns(given(), name, &sp, nullptr);
    }
    OptimizedDataFrame order(const char *name, int32_t median, double q) const {
        const pandrs_hip_window_quantile_spec sp{PANDRS_HIP_WINDOW_KIND_EXPANDING, median, 0, (int64_t)cfg_.min_periods, 0, 0, q};
        return df_.window_columns(given(), name, nullptr, &sp);
    }
};
inline DataFrameRollingOps OptimizedDataFrame::apply_rolling(const DataFrameRolling &config) const { return DataFrameRollingOps(*this, config); }
inline DataFrameExpandingOps OptimizedDataFrame::apply_expanding(const DataFrameExpanding &config) const { return DataFrameExpandingOps(*this, config); }

class GroupBy {
public:
    using Aggregation = std::tuple<std::string, AggregateOp, std::string>;      // (column, op, alias)
    const OptimizedDataFrame &df;
    std::vector<std::string> group_by_columns;
    bool create_multi_index = false;       // types.rs:54; set by group_by for >= 2 keys (grouping.rs:27, :107)

    GroupBy(const OptimizedDataFrame &d, std::vector<std::string> cols, bool multi_index = false)
        : df(d), group_by_columns(std::move(cols)), create_multi_index(multi_index) {}

    // aggregation.rs:763-871: key column(s) as strings, then one Float64 column per alias in request order
    OptimizedDataFrame aggregate(const std::vector<Aggregation> &aggregations) const {
        for (auto &a : aggregations)
            if (!df.contains_column(std::get<0>(a))) throw Error(Error::ColumnNotFound, std::get<0>(a));       // :770-774
        std::vector<pandrs_hip_column> keys, vals;
        std::vector<std::string> val_names;
        for (auto &k : group_by_columns) keys.push_back(df.view_of(k));
        std::vector<pandrs_hip_agg_spec> specs;
        for (auto &a : aggregations) {
            size_t vi = 0;
            while (vi < val_names.size() && val_names[vi] != std::get<0>(a)) vi++;
            if (vi == val_names.size()) { val_names.push_back(std::get<0>(a)); vals.push_back(df.view_of(std::get<0>(a))); }
            specs.push_back(pandrs_hip_agg_spec{(int32_t)vi, (int32_t)std::get<1>(a)});
        }
        int64_t g = 0;
        detail::check(pandrs_hip_groupby_agg(detail::context(), df.mem_space(), keys.data(), (int32_t)keys.size(), (int64_t)df.row_count(),
                                             vals.data(), (int32_t)vals.size(), specs.data(), (int32_t)specs.size(), &g));
        const size_t nk = keys.size(), na = specs.size();
        std::vector<std::vector<uint64_t>> kc(nk, std::vector<uint64_t>(g));
        std::vector<std::vector<uint8_t>> kn(nk, std::vector<uint8_t>(g));
        std::vector<std::vector<double>> oa(na, std::vector<double>(g));
        std::vector<uint64_t *> pk; std::vector<uint8_t *> pn; std::vector<double *> pa;
        for (auto &v : kc) pk.push_back(v.data());
        for (auto &v : kn) pn.push_back(v.data());
        for (auto &v : oa) pa.push_back(v.data());
        detail::check(pandrs_hip_groupby_fetch(detail::context(), PANDRS_HIP_MEM_HOST, pk.data(), pn.data(), pa.data()));
        OptimizedDataFrame result;
        std::vector<std::vector<std::string>> key_strings(nk, std::vector<std::string>(g));
        for (size_t k = 0; k < nk; k++)
            for (int64_t i = 0; i < g; i++) key_strings[k][i] = detail::key_string(keys[k].dtype, kc[k][i], kn[k][i] != 0);
        if (create_multi_index && nk > 1) {
            // :812-853: the key tuples become a StringMultiIndex (from_tuples refuses an empty list, multi_index.rs:160),
            // the result holds the aggregate columns only
            if (g == 0) throw Error(Error::Index, "Empty tuple list was passed");
            result.multi_index.assign((size_t)g, std::vector<std::string>(nk));
            for (int64_t i = 0; i < g; i++)
                for (size_t k = 0; k < nk; k++) result.multi_index[i][k] = key_strings[k][i];
            result.multi_index_names = group_by_columns;
        } else {
            for (size_t k = 0; k < nk; k++) result.add_column(group_by_columns[k], StringColumn(key_strings[k]));    // :856-860
        }
        for (size_t a = 0; a < na; a++) result.add_column(std::get<2>(aggregations[a]), Float64Column(oa[a]));  // :863-867
        return result;
    }
    // operations.rs:498-521: aliases "{col}_{op}"
    OptimizedDataFrame agg(const std::vector<std::pair<std::string, AggregateOp>> &aggs) const {
        std::vector<Aggregation> v;
        for (auto &a : aggs) v.emplace_back(a.first, a.second, a.first + "_" + op_name(a.second));
        return aggregate(v);
    }
    OptimizedDataFrame sum(const std::string &c) const { return agg({{c, AggregateOp::Sum}}); }
    OptimizedDataFrame mean(const std::string &c) const { return agg({{c, AggregateOp::Mean}}); }
    OptimizedDataFrame min(const std::string &c) const { return agg({{c, AggregateOp::Min}}); }
    OptimizedDataFrame max(const std::string &c) const { return agg({{c, AggregateOp::Max}}); }
    OptimizedDataFrame count(const std::string &c) const { return agg({{c, AggregateOp::Count}}); }
    OptimizedDataFrame std(const std::string &c) const { return agg({{c, AggregateOp::Std}}); }
    OptimizedDataFrame var(const std::string &c) const { return agg({{c, AggregateOp::Var}}); }
    OptimizedDataFrame median(const std::string &c) const { return agg({{c, AggregateOp::Median}}); }
    OptimizedDataFrame first(const std::string &c) const { return agg({{c, AggregateOp::First}}); }
    OptimizedDataFrame last(const std::string &c) const { return agg({{c, AggregateOp::Last}}); }
    OptimizedDataFrame nunique(const std::string &c) const { return agg({{c, AggregateOp::Nunique}}); }   // legacy GroupBy::nunique (src/dataframe/groupby.rs:386-393)

    // cumsum / cummax / cummin / cumcount / row_number / shift / diff / pct_change within the groups (pandrs_hip_grouped): for
    // every group the frame-level method of the same name over the group's rows in ascending row order, written at those rows;
    // vectors aligned with the frame's rows.  No closure and no sub-frames: one pandrs_hip_groupby_indices and one
    // pandrs_hip_grouped call each (this mirror regroups per call).  Errors before any device call: ColumnNotFound, Type (a
    // String or Boolean column); an empty frame gives empty vectors.
    std::vector<double> cumsum(const std::string &c) const { return grouped<double>(&c, PANDRS_HIP_GROUPED_CUM_SUM, 0, nullptr); }
    std::vector<double> cummax(const std::string &c) const { return grouped<double>(&c, PANDRS_HIP_GROUPED_CUM_MAX, 0, nullptr); }
    std::vector<double> cummin(const std::string &c) const { return grouped<double>(&c, PANDRS_HIP_GROUPED_CUM_MIN, 0, nullptr); }
    std::vector<size_t> cumcount(const std::string &c) const {
        const std::vector<int64_t> v = grouped<int64_t>(&c, PANDRS_HIP_GROUPED_CUM_COUNT, 0, nullptr);
        return std::vector<size_t>(v.begin(), v.end());
    }
    std::vector<size_t> row_number() const {
        const std::vector<int64_t> v = grouped<int64_t>(nullptr, PANDRS_HIP_GROUPED_ROW_NUMBER, 0, nullptr);
        return std::vector<size_t>(v.begin(), v.end());
    }
    std::vector<std::optional<double>> shift(const std::string &c, int32_t periods) const {
        std::vector<uint8_t> mask;
        const std::vector<double> v = grouped<double>(&c, PANDRS_HIP_GROUPED_SHIFT, periods, &mask);
        std::vector<std::optional<double>> out(v.size());
        for (size_t i = 0; i < v.size(); i++)
            if (!detail::bit_at(mask, i)) out[i] = v[i];
        return out;
    }
    std::vector<double> diff(const std::string &c, size_t periods) const { return grouped<double>(&c, PANDRS_HIP_GROUPED_DIFF, (int64_t)std::min(periods, df.row_count()), nullptr); }
    std::vector<double> pct_change(const std::string &c, size_t periods) const { return grouped<double>(&c, PANDRS_HIP_GROUPED_PCT_CHANGE, (int64_t)std::min(periods, df.row_count()), nullptr); }

    // the pub field `groups` (types.rs:52): HashMap<Vec<String>, Vec<usize>>, every list ascending
    std::map<std::vector<std::string>, std::vector<size_t>> groups(const char *null_string = "NULL") const {
        std::vector<pandrs_hip_column> keys;
        for (auto &k : group_by_columns) keys.push_back(df.view_of(k));
        int64_t g = 0;
        const int64_t n = (int64_t)df.row_count();
        detail::check(pandrs_hip_groupby_indices(detail::context(), df.mem_space(), keys.data(), (int32_t)keys.size(), n, &g));
        const size_t nk = keys.size();
        std::vector<std::vector<uint64_t>> kc(nk, std::vector<uint64_t>(g));
        std::vector<std::vector<uint8_t>> kn(nk, std::vector<uint8_t>(g));
        std::vector<uint64_t *> pk; std::vector<uint8_t *> pn;
        for (auto &v : kc) pk.push_back(v.data());
        for (auto &v : kn) pn.push_back(v.data());
        std::vector<int64_t> off(g + 1), rows(n);
        detail::check(pandrs_hip_groupby_indices_fetch(detail::context(), PANDRS_HIP_MEM_HOST, pk.data(), pn.data(), off.data(), rows.data()));
        std::map<std::vector<std::string>, std::vector<size_t>> out;
        for (int64_t i = 0; i < g; i++) {
            std::vector<std::string> key;
            for (size_t k = 0; k < nk; k++) key.push_back(detail::key_string(keys[k].dtype, kc[k][i], kn[k][i] != 0, null_string));
            auto &v = out[key];
            v.insert(v.end(), rows.begin() + off[i], rows.begin() + off[i + 1]);
        }
        return out;
    }
    // CustomAggregation / aggregate_custom (types.rs:58-67, aggregation.rs:391-497): host closure over the
    // group's non-null values (Int64 cast to f64); the groups come from the device
    OptimizedDataFrame custom(const std::string &column, const std::string &result_name, const std::function<double(const std::vector<double> &)> &fn) const {
        if (!df.contains_column(column)) throw Error(Error::ColumnNotFound, column);
        const Column &c = df.column(column);
        if (c.index() > 1) throw Error(Error::OperationFailed, "column '" + column + "' is not numeric");
        auto gs = groups();
        OptimizedDataFrame result;
        for (size_t k = 0; k < group_by_columns.size(); k++) {
            std::vector<std::string> strs;
            for (auto &kv : gs) strs.push_back(kv.first[k]);
            result.add_column(group_by_columns[k], StringColumn(strs));
        }
        std::vector<double> vals;
        for (auto &kv : gs) {
            std::vector<double> v;
            for (size_t r : kv.second) {
                if (c.index() == 0) { auto &x = std::get<Int64Column>(c); if (!detail::bit_at(x.null_mask, r)) v.push_back((double)x.data[r]); }
                else { auto &x = std::get<Float64Column>(c); if (!detail::bit_at(x.null_mask, r)) v.push_back(x.data[r]); }
            }
            vals.push_back(fn(v));
        }
        result.add_column(result_name, Float64Column(vals));
        return result;
    }

    // operations.rs:51-74: keep the rows of the groups whose sub-frame passes filter_fn
    OptimizedDataFrame filter(const std::function<bool(const OptimizedDataFrame &)> &filter_fn) const {
        std::vector<int64_t> keep;
        for (auto &kv : groups()) {
            std::vector<int64_t> rows(kv.second.begin(), kv.second.end());
            if (filter_fn(df.filter_by_indices(rows))) keep.insert(keep.end(), rows.begin(), rows.end());
        }
        return df.filter_by_indices(keep);
    }
    // operations.rs:132-276: transform_fn(group sub-frame) -> frame for every group, results concatenated
    // column by column after the first result's schema (columns matched by position and type)
    OptimizedDataFrame transform(const std::function<OptimizedDataFrame(const OptimizedDataFrame &)> &transform_fn) const {
        std::vector<OptimizedDataFrame> outs;
        for (auto &kv : groups()) outs.push_back(transform_fn(df.filter_by_indices(std::vector<int64_t>(kv.second.begin(), kv.second.end()))));
        OptimizedDataFrame result;
        if (outs.empty()) return result;
        const OptimizedDataFrame &tmpl = outs[0];
        for (size_t ci = 0; ci < tmpl.columns.size(); ci++) {
            Column acc = tmpl.columns[ci];
            std::visit([&](auto &a) {
                using T = std::decay_t<decltype(a)>;
                std::vector<bool> nulls;
                auto push_nulls = [&](const T &x) { for (size_t i = 0; i < x.len(); i++) nulls.push_back(detail::bit_at(x.null_mask, i)); };
                push_nulls(a);
                for (size_t d = 1; d < outs.size(); d++) {
                    if (ci >= outs[d].columns.size() || !std::holds_alternative<T>(outs[d].columns[ci])) continue;
                    const T &x = std::get<T>(outs[d].columns[ci]);
                    if constexpr (std::is_same_v<T, StringColumn>) a.indices.insert(a.indices.end(), x.indices.begin(), x.indices.end());
                    else if constexpr (std::is_same_v<T, BooleanColumn>) {
                        std::vector<bool> v(a.length + x.length);
                        for (size_t i = 0; i < a.length; i++) v[i] = a.get(i);
                        for (size_t i = 0; i < x.length; i++) v[a.length + i] = x.get(i);
                        a = BooleanColumn(v);
                    } else a.data.insert(a.data.end(), x.data.begin(), x.data.end());
                    push_nulls(x);
                }
                a.null_mask = detail::create_bitmask(nulls);
            }, acc);
            result.add_column(tmpl.column_names[ci], std::move(acc));
        }
        return result;
    }

    static std::string op_name(AggregateOp op) {
        static const char *names[] = {"sum", "mean", "min", "max", "count", "std", "var", "median", "first", "last", "custom", "nunique"};
        return names[(int)op];
    }

private:
    // the grouping, then one pandrs_hip_grouped call (op = pandrs_hip_grouped_op; column == nullptr: ROW_NUMBER) -> its cells
    // (T = int64_t for CUM_COUNT and ROW_NUMBER, double otherwise), and the null bitmap when `mask` is given
    template <typename T>
    std::vector<T> grouped(const std::string *column, int32_t op, int64_t periods, std::vector<uint8_t> *mask) const {
        if (column && df.column(*column).index() > 1) throw Error(Error::Type, "Column '" + *column + "' is not a numeric type");
        const size_t n = df.row_count();
        std::vector<T> out(n);
        if (mask) mask->assign((n + 7) / 8, 0);
        if (n) {
            std::vector<pandrs_hip_column> keys;
            for (auto &k : group_by_columns) keys.push_back(df.view_of(k));
            int64_t g = 0;
            detail::check(pandrs_hip_groupby_indices(detail::context(), df.mem_space(), keys.data(), (int32_t)keys.size(), (int64_t)n, &g));
            pandrs_hip_column v{};
            if (column) v = df.view_of(*column);
            detail::check(pandrs_hip_grouped(detail::context(), df.mem_space(), column ? &v : nullptr, (int64_t)n, op, periods, PANDRS_HIP_MEM_HOST,
                                             out.data(), mask ? mask->data() : nullptr, nullptr));
        }
        return out;
    }
};

inline GroupBy OptimizedDataFrame::group_by(const std::vector<std::string> &cols) const { return group_by_with_options(cols, true); }
inline GroupBy OptimizedDataFrame::group_by_with_options(const std::vector<std::string> &cols, bool as_multi_index) const {
    for (auto &c : cols) if (!contains_column(c)) throw Error(Error::ColumnNotFound, c);       // grouping.rs:53-57
    return GroupBy(*this, cols, as_multi_index && cols.size() > 1);                              // grouping.rs:107
}
inline std::map<std::string, OptimizedDataFrame> OptimizedDataFrame::par_groupby(const std::vector<std::string> &cols) const {
    for (auto &c : cols) if (!contains_column(c)) throw Error(Error::ColumnNotFound, c);
    std::map<std::string, std::vector<int64_t>> merged;           // parts joined with "_" (:186), a null part is "NA" (:158)
    for (auto &kv : GroupBy(*this, cols).groups("NA")) {
        std::string name;
        for (size_t i = 0; i < kv.first.size(); i++) name += (i ? "_" : "") + kv.first[i];
        auto &v = merged[name];
        v.insert(v.end(), kv.second.begin(), kv.second.end());
    }
    std::map<std::string, OptimizedDataFrame> out;
    for (auto &kv : merged) {
        std::vector<int64_t> rows = kv.second;
        std::sort(rows.begin(), rows.end());
        out.emplace(kv.first, filter_by_indices(rows));
    }
    return out;
}

// ---- LazyFrame (lazy.rs:98-170): the two operations on the accelerated path ---------------------------------
class LazyFrame {
public:
    explicit LazyFrame(OptimizedDataFrame df) : source_(std::move(df)) {}
    LazyFrame &aggregate(std::vector<std::string> group_by, std::vector<GroupBy::Aggregation> aggregations) {
        ops_.push_back(Op{true, std::move(group_by), std::move(aggregations), nullptr, "", "", JoinType::Inner});
        return *this;
    }
    LazyFrame &join(const OptimizedDataFrame &right, const std::string &left_on, const std::string &right_on, JoinType how) {
        ops_.push_back(Op{false, {}, {}, std::make_shared<OptimizedDataFrame>(right), left_on, right_on, how});
        return *this;
    }
    OptimizedDataFrame execute() const {
        OptimizedDataFrame df = source_;
        for (size_t oi = 0; oi < ops_.size(); oi++) {
            const Op &op = ops_[oi];
            if (op.is_aggregate) {
                for (auto &a : op.aggregations) {                   // lazy.rs:377-382: only these five ops
                    const AggregateOp o = std::get<1>(a);
                    if (o != AggregateOp::Sum && o != AggregateOp::Mean && o != AggregateOp::Min && o != AggregateOp::Max && o != AggregateOp::Count)
                        throw Error(Error::OperationFailed, "Aggregation operation " + GroupBy::op_name(o) + " is not supported in LazyFrame");
                }
                // the arm builds its frame inline and never a multi-index: key columns always (lazy.rs:390-394;
                // tests/optimized_groupby_test.rs:184 asserts 3 columns for two keys)
                df = df.group_by_with_options(op.group_by, false).aggregate(op.aggregations);
            } else {
                // Join(Inner) immediately followed by Aggregate([g], [(v, Sum, alias)]) with v a left column and g a right
                // column (lazy.rs:405-425 then :186) = BASELINE config 5: ONE fused device operator, no joined rows
                if (op.how == JoinType::Inner && oi + 1 < ops_.size() && ops_[oi + 1].is_aggregate) {
                    OptimizedDataFrame fused;
                    if (fused_join_groupby_sum(df, *op.right, op.left_on, op.right_on, ops_[oi + 1], fused)) {
                        df = std::move(fused);
                        oi++;
                        continue;
                    }
                }
                switch (op.how) {                                   // lazy.rs:405-425
                case JoinType::Inner: df = df.inner_join(*op.right, op.left_on, op.right_on); break;
                case JoinType::Left: df = df.left_join(*op.right, op.left_on, op.right_on); break;
                case JoinType::Right: df = df.right_join(*op.right, op.left_on, op.right_on); break;
                default: df = df.outer_join(*op.right, op.left_on, op.right_on);
                }
            }
        }
        return df;
    }
private:
    struct Op {
        bool is_aggregate;
        std::vector<std::string> group_by;
        std::vector<GroupBy::Aggregation> aggregations;
        std::shared_ptr<OptimizedDataFrame> right;
        std::string left_on, right_on;
        JoinType how;
    };
    // the shape test of hip_shim.rs `lazy_join_groupby_sum_hip` (same conditions, same result frame)
    static bool fused_join_groupby_sum(const OptimizedDataFrame &left, const OptimizedDataFrame &right, const std::string &left_on,
                                       const std::string &right_on, const Op &agg, OptimizedDataFrame &out) {
        if (agg.group_by.size() != 1 || agg.aggregations.size() != 1 || std::get<1>(agg.aggregations[0]) != AggregateOp::Sum) return false;
        const std::string &group_col = agg.group_by[0], &value_col = std::get<0>(agg.aggregations[0]), &alias = std::get<2>(agg.aggregations[0]);
        if (!left.contains_column(left_on) || !right.contains_column(right_on)) return false;     // the join arm throws ColumnNotFound
        if (value_col == left_on || !left.contains_column(value_col) || left.contains_column(group_col)) return false;
        std::string right_name;
        const std::string suffix = "_right";
        if (group_col.size() > suffix.size() && group_col.compare(group_col.size() - suffix.size(), suffix.size(), suffix) == 0 &&
            left.contains_column(group_col.substr(0, group_col.size() - suffix.size())) && right.contains_column(group_col.substr(0, group_col.size() - suffix.size())))
            right_name = group_col.substr(0, group_col.size() - suffix.size());               // join.rs:478-482
        else if (right.contains_column(group_col)) right_name = group_col;
        else return false;
        if (right_name == right_on) return false;
        const Column &lk = left.column(left_on), &lv = left.column(value_col), &rk = right.column(right_on), &rg = right.column(right_name);
        if (lk.index() != rk.index() || lv.index() > 1 || rg.index() == 3) return false;
        if (std::visit([](auto &x) { return !x.null_mask.empty(); }, rg)) return false;       // a null g would surface as the join's fill value (join.rs:304-307)
        const bool dev = left.is_resident() && right.is_resident();
        pandrs_hip_column a = dev ? left.view_of(left_on) : detail::view(lk), b = dev ? left.view_of(value_col) : detail::view(lv),
                          c = dev ? right.view_of(right_on) : detail::view(rk), d = dev ? right.view_of(right_name) : detail::view(rg);
        int64_t g = 0;
        detail::check(pandrs_hip_join_groupby_sum(detail::context(), dev ? PANDRS_HIP_MEM_DEVICE : PANDRS_HIP_MEM_HOST, &a, &b, (int64_t)left.row_count(), &c, &d,
                                                  (int64_t)right.row_count(), &g));
        std::vector<uint64_t> cells(g); std::vector<uint8_t> nulls(g); std::vector<double> sums(g);
        uint64_t *pk[1] = {cells.data()}; uint8_t *pn[1] = {nulls.data()}; double *pa[1] = {sums.data()};
        detail::check(pandrs_hip_groupby_fetch(detail::context(), PANDRS_HIP_MEM_HOST, pk, pn, pa));
        std::vector<std::string> strs(g);
        for (int64_t i = 0; i < g; i++) strs[i] = detail::key_string(d.dtype, cells[i], nulls[i] != 0);
        out.add_column(group_col, StringColumn(strs));
        out.add_column(alias, Float64Column(sums));
        return true;
    }
    OptimizedDataFrame source_;
    std::vector<Op> ops_;
};

}  // namespace pandrs
