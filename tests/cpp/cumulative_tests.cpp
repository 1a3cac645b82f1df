// PandasCompatExt::cumsum / cumprod / cummax / cummin / shift / pct_change / diff / cumcount
// (src/dataframe/pandas_compat/functions.rs:280-342, :514-541, :2081-2094) through the C++ host mirror
// (include/pandrs_hip.hpp) over libpandrs_hip.so: the reference's known answers (functions.rs:4411-4447, :4547-4573,
// :6580-6595), host and resident, and the Int64 / null-mask extensions of pandrs_hip.h.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "pandrs_hip.hpp"

using namespace pandrs;

static int g_failed = 0, g_run = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("    CHECK failed: %s  (%s:%d)\n", #cond, __FILE__, __LINE__); g_failed++; } } while (0)
#define RUN(fn) do { g_run++; std::printf("test %s\n", #fn); try { fn(); } catch (const std::exception &e) { std::printf("    threw: %s\n", e.what()); g_failed++; } } while (0)

// the reference's create_test_df (functions.rs:4327-4355)
static OptimizedDataFrame test_df(bool resident) {
    OptimizedDataFrame df;
    df.add_column("a", Float64Column(std::vector<double>{1.0, 2.0, 3.0, 4.0, 5.0}));
    df.add_column("b", Float64Column(std::vector<double>{5.0, 4.0, 3.0, 2.0, 1.0}));
    df.add_column("name", StringColumn(std::vector<std::string>{"Alice", "Bob", "Charlie", "David", "Eve"}));
    df.add_column("flag", BooleanColumn(std::vector<bool>(5, true)));
    if (resident) df.make_resident();
    return df;
}

static OptimizedDataFrame one(const std::vector<double> &x, bool resident) {
    OptimizedDataFrame df;
    df.add_column("x", Float64Column(x));
    if (resident) df.make_resident();
    return df;
}

static void test_errors_before_any_device_call() {
    auto df = test_df(false);
    try { df.cumsum("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.shift("nope", 1); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.cumprod("name"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.cummax("flag"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type && std::string(e.what()) == "Column 'flag' is not a numeric type"); }
    try { df.cumcount("name"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.diff("name", 1); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.pct_change("flag", 1); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    OptimizedDataFrame empty;
    empty.add_column("v", Float64Column(std::vector<double>{}));
    CHECK(empty.cumsum("v").empty() && empty.cummin("v").empty() && empty.cumcount("v").empty() && empty.shift("v", 1).empty() &&
          empty.diff("v", 1).empty() && empty.pct_change("v", 2).empty());
    CHECK(PANDRS_HIP_CUM_SUM == 0 && PANDRS_HIP_CUM_PROD == 1 && PANDRS_HIP_CUM_MAX == 2 && PANDRS_HIP_CUM_MIN == 3 && PANDRS_HIP_CUM_COUNT == 4);
    CHECK(PANDRS_HIP_LAG_SHIFT == 0 && PANDRS_HIP_LAG_DIFF == 1 && PANDRS_HIP_LAG_PCT_CHANGE == 2);
}

static void test_known_answers() {
    for (int res = 0; res < 2; res++) {
        auto df = test_df(res);
        CHECK(df.cumsum("a") == (std::vector<double>{1.0, 3.0, 6.0, 10.0, 15.0}));                                // :4411
        CHECK(one({1.0, 2.0, 3.0, 4.0}, res).cumprod("x") == (std::vector<double>{1.0, 2.0, 6.0, 24.0}));         // :4417
        CHECK(df.cummax("b") == (std::vector<double>{5.0, 5.0, 5.0, 5.0, 5.0}));                                  // :4428
        CHECK(df.cummin("b") == (std::vector<double>{5.0, 4.0, 3.0, 2.0, 1.0}));                                  // :4434
        auto s = df.shift("a", 1);                                                                                // :4440
        CHECK(s.size() == 5 && !s[0] && s[1] == 1.0 && s[2] == 2.0 && s[4] == 4.0);
        auto back = df.shift("a", -2);
        CHECK(back[0] == 3.0 && back[2] == 5.0 && !back[3] && !back[4]);
        auto p = df.pct_change("a", 1);                                                                           // :4547
        CHECK(std::isnan(p[0]) && p[1] == (2.0 - 1.0) / 1.0 && p[2] == (3.0 - 2.0) / 2.0);
        auto d = df.diff("a", 1);                                                                                 // :4555
        CHECK(std::isnan(d[0]) && d[1] == 1.0 && d[2] == 1.0 && d[3] == 1.0 && d[4] == 1.0);
        auto d2 = df.diff("a", 2);                                                                                // :4564
        CHECK(std::isnan(d2[0]) && std::isnan(d2[1]) && d2[2] == 2.0 && d2[3] == 2.0 && d2[4] == 2.0);
        auto far = df.diff("a", 99);
        CHECK(far.size() == 5 && std::isnan(far[0]) && std::isnan(far[4]));
        CHECK(one({1.0, NAN, 3.0, NAN, 5.0}, res).cumcount("x") == (std::vector<size_t>{1, 1, 2, 2, 3}));         // :6580
    }
}

static void test_quirks_int64_and_null_masks() {
    for (int res = 0; res < 2; res++) {
        auto m = one({NAN, 2.0, NAN, 1.0, 3.0}, res).cummax("x");                 // a leading NaN: the fold's -inf shows
        CHECK(std::isinf(m[0]) && m[0] < 0 && m[1] == 2.0 && m[2] == 2.0 && m[3] == 2.0 && m[4] == 3.0);
        auto z = one({-0.0, -0.0, -0.0}, res).cumsum("x");                        // the fold starts from +0.0
        CHECK(z[0] == 0.0 && !std::signbit(z[0]) && !std::signbit(z[2]));
        auto s = one({1.0, NAN, 3.0}, res).cumsum("x");
        CHECK(s[0] == 1.0 && std::isnan(s[1]) && std::isnan(s[2]));
        auto pc = one({-0.0, 5.0, 0.0, 1.0}, res).pct_change("x", 1);             // prev == 0.0 holds for -0.0 too
        CHECK(std::isnan(pc[0]) && std::isnan(pc[1]) && pc[2] == -1.0 && std::isnan(pc[3]));
        auto r = one({1e-200, 1e200, 1e200, 1e-200}, res).cumprod("x");           // rows 1 .. 2 alone overflow
        CHECK(r[0] == 1e-200 && std::fabs(r[1] - 1.0) < 1e-15 && std::fabs(r[2] / 1e200 - 1.0) < 1e-15 && std::fabs(r[3] - 1.0) < 1e-15);
        auto o = one({1e200, 1e200, 1e-200, 1e-200, 0.0, 2.0}, res).cumprod("x"); // sticky after the overflow, NaN after the 0
        CHECK(o[0] == 1e200 && std::isinf(o[1]) && std::isinf(o[2]) && std::isinf(o[3]) && std::isnan(o[4]) && std::isnan(o[5]));
        OptimizedDataFrame df;
        df.add_column("i", Int64Column::with_nulls({7, 100, 2, -3, 1}, {false, true, false, false, false}));
        if (res) df.make_resident();
        auto cs = df.cumsum("i");
        CHECK(cs[0] == 7.0 && std::isnan(cs[1]) && cs[2] == 9.0 && cs[3] == 6.0 && cs[4] == 7.0);
        CHECK(df.cumcount("i") == (std::vector<size_t>{1, 1, 2, 3, 4}));
        auto sh = df.shift("i", 1);
        CHECK(!sh[0] && sh[1] == 7.0 && !sh[2] && sh[3] == 2.0 && sh[4] == -3.0);
        auto di = df.diff("i", 1);
        CHECK(std::isnan(di[0]) && std::isnan(di[1]) && std::isnan(di[2]) && di[3] == -5.0 && di[4] == 4.0);
    }
    const std::vector<double> x = {1.0, 2.0, 3.0};
    const pandrs_hip_column col{x.data(), nullptr, PANDRS_HIP_F64, 0};
    double out[3] = {0, 0, 0};
    int64_t nulls = -1;
    CHECK(pandrs_hip_cumulative(detail::context(), PANDRS_HIP_MEM_HOST, &col, 3, 5, PANDRS_HIP_MEM_HOST, out, nullptr, &nulls) == PANDRS_HIP_ERR_INVALID_ARGUMENT);
    CHECK(pandrs_hip_lag(detail::context(), PANDRS_HIP_MEM_HOST, &col, 3, PANDRS_HIP_LAG_DIFF, -1, PANDRS_HIP_MEM_HOST, out, nullptr, &nulls) == PANDRS_HIP_ERR_INVALID_ARGUMENT);
    CHECK(pandrs_hip_cumulative(detail::context(), PANDRS_HIP_MEM_HOST, &col, 3, PANDRS_HIP_CUM_SUM, PANDRS_HIP_MEM_HOST, out, nullptr, &nulls) == PANDRS_HIP_OK);
    CHECK(out[0] == 1.0 && out[1] == 3.0 && out[2] == 6.0 && nulls == 0);
}

int main() {
    RUN(test_errors_before_any_device_call);
    int32_t n_dev = 0;
    if (pandrs_hip_init(nullptr) != PANDRS_HIP_OK || pandrs_hip_device_count(&n_dev) != PANDRS_HIP_OK || n_dev == 0) {
        std::printf("%d tests, %d failed checks\n", g_run, g_failed);
        std::fprintf(stderr, "no HIP device available: %s\n", pandrs_hip_last_error());
        return g_failed ? 2 : 1;
    }
    RUN(test_known_answers);
    RUN(test_quirks_int64_and_null_masks);
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
