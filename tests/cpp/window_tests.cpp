// DataFrameWindowExt::{rolling, expanding, ewm} (src/dataframe/window.rs:13-160 over src/series/window.rs) through the
// C++ host mirror (include/pandrs_hip.hpp) over libpandrs_hip.so.  The expected values are the reference's loops restated
// here: a window's non-null values folded in row order from -0.0, EWM's recurrence line by line.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "pandrs_hip.hpp"

using namespace pandrs;

static int g_failed = 0, g_run = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("    CHECK failed: %s  (%s:%d)\n", #cond, __FILE__, __LINE__); g_failed++; } } while (0)
#define RUN(fn) do { g_run++; std::printf("test %s\n", #fn); try { fn(); } catch (const std::exception &e) { std::printf("    threw: %s\n", e.what()); g_failed++; } } while (0)

static OptimizedDataFrame sample_frame() {
    OptimizedDataFrame df;
    df.add_column("id", Int64Column({1, 2, 3, 4, 5, 6, 7}));
    df.add_column("x", Float64Column::with_nulls({1.0, 2.0, 0.5, 4.0, -0.0, 6.0, 7.25}, {false, false, true, false, false, false, false}));
    df.add_column("s", StringColumn({"a", "b", "c", "d", "e", "f", "g"}));
    df.add_column("b", BooleanColumn({true, false, true, false, true, false, true}));
    return df;
}

static bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || (a == b && std::signbit(a) == std::signbit(b)); }

static void test_errors_before_any_device_call() {
    auto df = sample_frame();
    try { df.rolling(3, "nope", "mean"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.rolling(3, "s", "mean"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnTypeMismatch); }
    try { df.expanding(1, "b", "sum"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnTypeMismatch); }
    try { df.rolling(0, "x", "mean"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    try { df.rolling(2, "x", "median"); CHECK(false); }
    catch (const Error &e) { CHECK(e.kind == Error::InvalidValue && std::string(e.what()) == "Unsupported rolling operation: median"); }
    try { df.ewm("x", "sum", nullptr, nullptr); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    const double bad = 1.5;
    try { df.ewm("x", "mean", nullptr, &bad); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    try { df.ewm("x", "sum", nullptr, &bad); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    try { df.rolling(2, "x", "sum", "id"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::DuplicateColumnName); }
    OptimizedDataFrame empty;
    empty.add_column("v", Float64Column(std::vector<double>{}));
    auto r = empty.rolling(3, "v", "Sum");
    CHECK(r.column_names == (std::vector<std::string>{"v", "v_Sum"}) && r.row_count() == 0);
}

static void test_windows_match_the_reference_loop() {
    for (int resident = 0; resident < 2; resident++) {
        auto df = sample_frame();
        if (resident) df.make_resident();
        // x = 1, 2, None, 4, -0.0, 6, 7.25
        auto r = df.rolling(3, "x", "SUM", "", 1);
        CHECK(r.column_names.back() == "x_SUM" && r.column_count() == 5);
        const std::vector<double> sum = {-0.0 + 1.0, (-0.0 + 1.0) + 2.0, (-0.0 + 1.0) + 2.0, -0.0 + 2.0 + 4.0, (-0.0 + 4.0) + -0.0,
                                         ((-0.0 + 4.0) + -0.0) + 6.0, ((-0.0 + -0.0) + 6.0) + 7.25};
        auto &got = std::get<Float64Column>(r.column("x_SUM"));
        CHECK(got.null_mask.empty());
        for (size_t i = 0; i < sum.size(); i++) CHECK(same(got.data[i], sum[i]));
        // the default min_periods (= 3): rows 0..4 hold fewer than three values
        auto m = std::get<Float64Column>(df.rolling(3, "x", "mean").column("x_mean")).data;
        CHECK(std::isnan(m[0]) && std::isnan(m[1]) && std::isnan(m[2]) && std::isnan(m[3]) && std::isnan(m[4]));
        CHECK(same(m[5], ((-0.0 + 4.0) + -0.0 + 6.0) / 3.0) && same(m[6], ((-0.0 + -0.0) + 6.0 + 7.25) / 3.0));
        // centred count: windows [0,3), [0,3), [1,4), [2,5), [3,6), [4,7), [5,7)
        auto c = std::get<Float64Column>(df.rolling(3, "x", "count", "n", 0, true).column("n")).data;
        CHECK(c == (std::vector<double>{2, 2, 2, 2, 3, 3, 2}));
        auto mx = std::get<Float64Column>(df.rolling(2, "id", "max", "", 1).column("id_max")).data;
        CHECK(mx == (std::vector<double>{1, 2, 3, 4, 5, 6, 7}));
        auto ex = std::get<Float64Column>(df.expanding(2, "x", "min").column("x_min")).data;
        CHECK(std::isnan(ex[0]) && ex[1] == 1.0 && ex[2] == 1.0 && ex[3] == 1.0 && same(ex[4], -0.0) && same(ex[6], -0.0));
        auto sd = std::get<Float64Column>(df.rolling(2, "id", "std", "sd", -1, false, 0).column("sd")).data;
        CHECK(std::isnan(sd[0]) && sd[1] == 0.5 && sd[6] == 0.5);
        // EWM mean, alpha 0.5 (span 3): x0 as itself, then 0.5 v + 0.5 y; a null row repeats y
        const size_t span = 3;
        auto e = std::get<Float64Column>(df.ewm("x", "mean", &span, nullptr, "em").column("em")).data;
        double y = 1.0;
        CHECK(e[0] == 1.0);
        y = 0.5 * 2.0 + 0.5 * y;
        CHECK(e[1] == y && e[2] == y);
        y = 0.5 * 4.0 + 0.5 * y;
        CHECK(std::fabs(e[3] - y) <= 1e-12 * 8);
        const double alpha = 0.5;
        auto v = std::get<Float64Column>(df.ewm("x", "var", nullptr, &alpha).column("x_var")).data;
        auto s = std::get<Float64Column>(df.ewm("x", "std", nullptr, &alpha).column("x_std")).data;
        CHECK(std::isnan(v[0]) && std::isnan(s[0]));
        for (size_t i = 1; i < v.size(); i++) CHECK(same(v[i], s[i] * s[i]));
        CHECK(std::fabs(s[1] - std::sqrt(0.5 * (0.0 + 0.5 * 1.0 * 1.0))) <= 1e-12 * 8);
    }
}

int main() {
    RUN(test_errors_before_any_device_call);
    int32_t n_dev = 0;
    if (pandrs_hip_init(nullptr) != PANDRS_HIP_OK || pandrs_hip_device_count(&n_dev) != PANDRS_HIP_OK || n_dev == 0) {
        std::printf("%d tests, %d failed checks\n", g_run, g_failed);
        std::fprintf(stderr, "no HIP device available: %s\n", pandrs_hip_last_error());
        return g_failed ? 2 : 1;
    }
    RUN(test_windows_match_the_reference_loop);
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
