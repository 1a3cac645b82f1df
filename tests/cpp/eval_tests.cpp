// Derived columns through the C++ host mirror (include/pandrs_hip.hpp) over libpandrs_hip.so: pandrs_hip_eval_check without a
// device, then PandasCompatExt::add_scalar / col_mul / clip / where_cond / round / coalesce / sign / normalize and a raw fused
// program (src/dataframe/pandas_compat/functions.rs:237, :1079-1139, :2316-2337, :2819-2960, :3846-4014), host and resident.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "pandrs_hip.hpp"

using namespace pandrs;
using Op = OptimizedDataFrame::EvalOp;

static int g_failed = 0, g_run = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("    CHECK failed: %s  (%s:%d)\n", #cond, __FILE__, __LINE__); g_failed++; } } while (0)
#define RUN(fn) do { g_run++; std::printf("test %s\n", #fn); try { fn(); } catch (const std::exception &e) { std::printf("    threw: %s\n", e.what()); g_failed++; } } while (0)

static OptimizedDataFrame test_df(bool resident) {
    OptimizedDataFrame df;
    df.add_column("a", Float64Column(std::vector<double>{1.0, -2.5, NAN, 4.0, 5.5}));
    df.add_column("b", Int64Column(std::vector<int64_t>{5, 4, 3, 2, 1}));
    df.add_column("name", StringColumn(std::vector<std::string>{"Alice", "Bob", "Charlie", "David", "Eve"}));
    df.add_column("flag", BooleanColumn(std::vector<bool>{true, false, true, false, true}));
    if (resident) df.make_resident();
    return df;
}

static const std::vector<double> &f64(const OptimizedDataFrame &df, const std::string &name) { return std::get<Float64Column>(df.column(name)).data; }

static void test_errors_before_any_device_call() {
    auto df = test_df(false);
    try { df.add_scalar("nope", 1.0); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.clip("name", 0.0, 1.0); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.sqrt("flag"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type && std::string(e.what()) == "Column 'flag' is not a numeric type"); }
    try { df.col_add("a", "b", "a"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::DuplicateColumnName); }
    try { df.col_add("a", "name", "c"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.where_cond("a", {true, false}, 0.0); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    try { df.sign("name"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.eval({"a"}, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_ADD, 0}}); CHECK(false); } catch (const Error &e) {
        CHECK(e.kind == Error::InvalidValue && std::string(e.what()).find("op 1") != std::string::npos);
    }
    try { df.eval({"a"}, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_ISNAN, 0}}); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    try { df.eval_mask({"a"}, {{PANDRS_HIP_EVAL_COL, 0}}); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    try { df.eval({"a", "flag"}, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_COL, 1}, {PANDRS_HIP_EVAL_MUL, 0}}); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    // the validator itself: the result type, the depth, the limits
    const int32_t dts[3] = {PANDRS_HIP_F64, PANDRS_HIP_BOOLBITS, PANDRS_HIP_U32CODE};
    const int32_t ops[7] = {PANDRS_HIP_EVAL_COL, PANDRS_HIP_EVAL_COL, PANDRS_HIP_EVAL_MUL, PANDRS_HIP_EVAL_CONST, PANDRS_HIP_EVAL_ADD, PANDRS_HIP_EVAL_CONST, PANDRS_HIP_EVAL_GT};
    const double args[7] = {0, 0, 0, 1.0, 0, 0.0, 0};
    int32_t is_mask = -1, depth = -1;
    CHECK(pandrs_hip_eval_check(dts, 3, ops, args, 7, &is_mask, &depth) == PANDRS_HIP_OK && is_mask == 1 && depth == 2);
    CHECK(pandrs_hip_eval_check(dts, 3, ops, args, 5, &is_mask, &depth) == PANDRS_HIP_OK && is_mask == 0 && depth == 2);
    CHECK(pandrs_hip_eval_check(dts, 3, ops, args, 6, &is_mask, &depth) == PANDRS_HIP_ERR_INVALID_ARGUMENT);       // two entries left
    const double col2[1] = {2.0};
    CHECK(pandrs_hip_eval_check(dts, 3, ops, col2, 1, nullptr, nullptr) == PANDRS_HIP_ERR_TYPE_MISMATCH);
    CHECK(pandrs_hip_eval_check(dts, 9, ops, args, 5, nullptr, nullptr) == PANDRS_HIP_ERR_INVALID_ARGUMENT);
    CHECK(pandrs_hip_eval_check(dts, 3, ops, args, 0, nullptr, nullptr) == PANDRS_HIP_ERR_INVALID_ARGUMENT);
    CHECK(pandrs_hip_eval(nullptr, PANDRS_HIP_MEM_HOST, nullptr, 1, 0, ops, args, 5, PANDRS_HIP_MEM_HOST, nullptr, nullptr, nullptr) == PANDRS_HIP_ERR_NOT_INITIALIZED);
    OptimizedDataFrame empty;
    empty.add_column("v", Float64Column(std::vector<double>{}));
    CHECK(empty.add_scalar("v", 1.0).row_count() == 0 && empty.sign("v").empty() && empty.eval_mask({"v"}, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_ISNAN, 0}}).empty());
    CHECK(PANDRS_HIP_EVAL_COL == 0 && PANDRS_HIP_EVAL_MIN == 8 && PANDRS_HIP_EVAL_SIGN == 17 && PANDRS_HIP_EVAL_NE == 23 && PANDRS_HIP_EVAL_SELECT == 30);
}

static void test_named_methods() {
    for (int res = 0; res < 2; res++) {
        auto df = test_df(res);
        auto r = df.add_scalar("a", 0.5);
        CHECK(r.column_names == df.column_names && f64(r, "a")[0] == 1.5 && f64(r, "a")[1] == -2.0 && std::isnan(f64(r, "a")[2]) && f64(r, "a")[4] == 6.0);
        r = df.col_mul("a", "b", "ab");
        CHECK(r.column_names.back() == "ab" && f64(r, "ab")[0] == 5.0 && f64(r, "ab")[1] == -10.0 && std::isnan(f64(r, "ab")[2]) && f64(r, "ab")[3] == 8.0);
        r = df.clip("a", 0.0, 4.5);                                           // a NaN cell clips to the bound
        CHECK(f64(r, "a") == (std::vector<double>{1.0, 0.0, 0.0, 4.0, 4.5}));
        r = df.where_cond("a", {true, false, true, false, true}, -1.0);
        CHECK(f64(r, "a")[0] == 1.0 && f64(r, "a")[1] == -1.0 && std::isnan(f64(r, "a")[2]) && f64(r, "a")[3] == -1.0 && f64(r, "a")[4] == 5.5);
        r = df.mask("a", {true, false, true, false, true}, -1.0);
        CHECK(f64(r, "a") == (std::vector<double>{-1.0, -2.5, -1.0, 4.0, -1.0}));
        r = df.round("a", 0);                                                 // half away from zero
        CHECK(f64(r, "a")[1] == -3.0 && f64(r, "a")[4] == 6.0);
        r = df.coalesce("a", "b", "c");
        CHECK(f64(r, "c") == (std::vector<double>{1.0, -2.5, 3.0, 4.0, 5.5}));
        r = df.fillna_zero("a");
        CHECK(f64(r, "a") == (std::vector<double>{1.0, -2.5, 0.0, 4.0, 5.5}));
        CHECK(df.sign("a") == (std::vector<int32_t>{1, -1, 0, 1, 1}));
        auto nz = df.normalize("b");
        CHECK(nz == (std::vector<double>{1.0, 0.75, 0.5, 0.25, 0.0}));
        r = df.floordiv("b", 2.0);
        CHECK(f64(r, "b") == (std::vector<double>{2.0, 2.0, 1.0, 1.0, 0.0}));
        // one fused call: a * b + 1 > 0 && flag
        auto m = df.eval_mask({"a", "b", "flag"}, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_COL, 1}, {PANDRS_HIP_EVAL_MUL, 0}, {PANDRS_HIP_EVAL_CONST, 1.0},
                                                   {PANDRS_HIP_EVAL_ADD, 0}, {PANDRS_HIP_EVAL_CONST, 0.0}, {PANDRS_HIP_EVAL_GT, 0}, {PANDRS_HIP_EVAL_COL, 2}, {PANDRS_HIP_EVAL_AND, 0}});
        CHECK(m == (std::vector<bool>{true, false, false, false, true}));
    }
    OptimizedDataFrame one;                                                   // no fused multiply-add: a * b + c is two roundings
    const double e = std::ldexp(1.0, -30);
    one.add_column("a", Float64Column(std::vector<double>{1.0 + e}));
    one.add_column("b", Float64Column(std::vector<double>{1.0 - e}));
    auto v = one.eval({"a", "b"}, {{PANDRS_HIP_EVAL_COL, 0}, {PANDRS_HIP_EVAL_COL, 1}, {PANDRS_HIP_EVAL_MUL, 0}, {PANDRS_HIP_EVAL_CONST, -1.0}, {PANDRS_HIP_EVAL_ADD, 0}});
    CHECK(v.size() == 1 && v[0] == 0.0);
}

int main() {
    RUN(test_errors_before_any_device_call);
    int32_t n_dev = 0;
    if (pandrs_hip_init(nullptr) != PANDRS_HIP_OK || pandrs_hip_device_count(&n_dev) != PANDRS_HIP_OK || n_dev == 0) {
        std::printf("%d tests, %d failed checks\n", g_run, g_failed);
        std::fprintf(stderr, "no HIP device available: %s\n", pandrs_hip_last_error());
        return g_failed ? 2 : 1;
    }
    RUN(test_named_methods);
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
