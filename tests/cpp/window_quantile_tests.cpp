// rolling_median, apply_rolling and apply_expanding (PandasCompatExt::rolling_median, helpers/window_ops.rs:206-240;
// DataFrameRollingOps / DataFrameExpandingOps::{median, quantile}, dataframe/enhanced_window.rs) through the C++ host
// mirror (include/pandrs_hip.hpp) over libpandrs_hip.so.  The device cases replay the reference's own known answers
// (tests/golden/window_quantile_known_answers.json, restated here) and a few windows sorted by hand.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "pandrs_hip.hpp"

using namespace pandrs;

static int g_failed = 0, g_run = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("    CHECK failed: %s  (%s:%d)\n", #cond, __FILE__, __LINE__); g_failed++; } } while (0)
#define RUN(fn) do { g_run++; std::printf("test %s\n", #fn); try { fn(); } catch (const std::exception &e) { std::printf("    threw: %s\n", e.what()); g_failed++; } } while (0)

static bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || (a == b && std::signbit(a) == std::signbit(b)); }
static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (!same(a[i], b[i])) return false;
    return true;
}
static const double NA = NAN;

static OptimizedDataFrame frame_of(const std::vector<double> &v) {
    OptimizedDataFrame df;
    df.add_column("a", Float64Column(v));
    return df;
}

static OptimizedDataFrame sample_frame() {
    OptimizedDataFrame df;
    df.add_column("id", Int64Column({1, 2, 3, 4, 5, 6, 7}));
    df.add_column("x", Float64Column::with_nulls({1.0, 2.0, 0.5, 4.0, -0.0, 6.0, 0.0}, {false, false, true, false, false, false, false}));
    df.add_column("s", StringColumn({"a", "b", "c", "d", "e", "f", "g"}));
    return df;
}

static void test_errors_before_any_device_call() {
    auto df = sample_frame();
    try { df.rolling_median("nope", 3); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.rolling_median("s", 3); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnTypeMismatch); }
    DataFrameRolling zero(0), three(3), missing(3), strings(3), twice(2);
    missing.columns({"x", "nope"});
    strings.columns({"s"});
    twice.columns({"x", "x"});
    try { df.apply_rolling(zero).median(); CHECK(false); }
    catch (const Error &e) { CHECK(e.kind == Error::InvalidValue && std::string(e.what()) == "Window size must be greater than 0"); }
    try { df.apply_rolling(three).quantile(1.5); CHECK(false); }
    catch (const Error &e) { CHECK(e.kind == Error::InvalidValue && std::string(e.what()) == "Quantile must be between 0 and 1"); }
    try { df.apply_rolling(three).quantile(-0.1); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    try { df.apply_rolling(three).quantile(NAN); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    try { df.apply_rolling(missing).median(); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.apply_rolling(strings).median(); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnTypeMismatch); }
    try { df.apply_rolling(twice).median(); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::DuplicateColumnName); }
    DataFrameExpanding ex(1);
    try { df.apply_expanding(ex).quantile(2.0); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    OptimizedDataFrame empty;
    empty.add_column("v", Float64Column(std::vector<double>{}));
    empty.add_column("t", StringColumn(std::vector<std::string>{}));
    auto r = empty.apply_rolling(three).median();
    CHECK(r.column_names == (std::vector<std::string>{"v", "t", "v_median"}) && r.row_count() == 0);
    CHECK(empty.apply_expanding(ex).quantile(0.5).column_names == (std::vector<std::string>{"v", "t", "v_quantile"}));
    CHECK(empty.rolling_median("v", 3).empty());
}

static std::vector<double> col(const OptimizedDataFrame &df, const std::string &name) { return std::get<Float64Column>(df.column(name)).data; }

static void test_known_answers_of_the_reference() {
    // functions.rs:6480-6494
    CHECK(same(frame_of({3.0, 1.0, 4.0, 1.0, 5.0}).rolling_median("a", 3), {NA, NA, 3.0, 1.0, 4.0}));
    // comprehensive_window_test.rs:44-47, :143-155
    std::vector<double> ten, nine;
    for (int i = 1; i <= 10; i++) ten.push_back(i);
    for (int i = 1; i <= 9; i++) nine.push_back(i);
    DataFrameRolling three(3);
    auto m = col(frame_of(ten).apply_rolling(three).median(), "a_median");
    CHECK(std::isnan(m[0]) && std::isnan(m[1]) && m[2] == 2.0 && m[3] == 3.0 && m[9] == 9.0);
    auto q50 = col(frame_of(nine).apply_rolling(three).quantile(0.5), "a_quantile");
    CHECK(q50[2] == 2.0 && q50[3] == 3.0);
    auto q75 = col(frame_of(nine).apply_rolling(three).quantile(0.75), "a_quantile");
    CHECK(q75[2] == 3.0 && q75[3] == 4.0);
    // window_test.rs:274-344: min_periods 2
    DataFrameRolling two_of_three(3);
    two_of_three.min_periods(2);
    CHECK(same(col(frame_of({10.0, 20.0, 30.0, 40.0, 50.0}).apply_rolling(two_of_three).median(), "a_median"), {NA, 15.0, 20.0, 30.0, 40.0}));
}

static void test_windows_sorted_by_hand() {
    for (int resident = 0; resident < 2; resident++) {
        auto df = sample_frame();
        if (resident) df.make_resident();
        // x = 1, 2, None, 4, -0.0, 6, 0.0; id = 1 .. 7
        DataFrameRolling r3(3);
        r3.min_periods(1);
        auto r = df.apply_rolling(r3).median();
        CHECK(r.column_names == (std::vector<std::string>{"id", "x", "s", "id_median", "x_median"}));
        CHECK(same(col(r, "x_median"), {1.0, 1.5, 1.5, 3.0, (-0.0 + 4.0) / 2.0, 4.0, 0.0}));
        CHECK(same(col(r, "id_median"), {1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 6.0}));
        // the zeros tie in row order: [-0.0, 6, 0.0] sorts to -0.0, 0.0, 6: the middle cell is +0.0; q = 0 reads -0.0
        DataFrameRolling z3(3);
        z3.columns({"x"});
        CHECK(same(col(df.apply_rolling(z3).median(), "x_median")[6], 0.0));
        CHECK(same(col(df.apply_rolling(z3).quantile(0.0), "x_quantile")[6], -0.0));
        // centred, window 40 (the general path): every window is [0, 7)
        DataFrameRolling wide(40);
        wide.min_periods(0).center(true).columns({"x"});
        auto w = col(df.apply_rolling(wide).median(), "x_median");            // sorted: -0.0 0.0 1 2 4 6 -> (1 + 2) / 2
        for (double v : w) CHECK(v == 1.5);
        DataFrameExpanding e2(2);
        e2.columns({"x"});
        CHECK(same(col(df.apply_expanding(e2).median(), "x_median"), {NA, 1.5, 1.5, 2.0, 1.5, 2.0, 1.5}));
        CHECK(same(col(df.apply_expanding(e2).quantile(0.5), "x_quantile"), {NA, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0}));   // round(0.5 (len-1)): half away
        CHECK(same(col(df.apply_expanding(e2).max(), "x_max"), {NA, 2.0, 2.0, 4.0, 4.0, 6.0, 6.0}));
        CHECK(same(df.rolling_median("id", 2, 1), {1.0, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5}));
        CHECK(same(df.rolling_median("x", 0), {1.0, 2.0, NA, 4.0, -0.0, 6.0, 0.0}));
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
    RUN(test_known_answers_of_the_reference);
    RUN(test_windows_sorted_by_hand);
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
