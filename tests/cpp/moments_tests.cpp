// PandasCompatExt's whole-column shape statistics (src/dataframe/pandas_compat/functions.rs:1617-1665, :2284-2314, :3571-3588,
// :4207-4224, :934-1022, :1583-1615; helpers/aggregations.rs:8-225) through the C++ host mirror (include/pandrs_hip.hpp) over
// libpandrs_hip.so: the reference's own tests of these methods (functions.rs:5011-5112, :5866-5970, :6868-6895, :7801-7820,
// :7979-8006, :8210-8222, :8637-8668, :8699-8790) with their inputs and asserted values.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "pandrs_hip.hpp"

using namespace pandrs;

static int g_failed = 0, g_run = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("    CHECK failed: %s  (%s:%d)\n", #cond, __FILE__, __LINE__); g_failed++; } } while (0)
#define RUN(fn) do { g_run++; std::printf("test %s\n", #fn); try { fn(); } catch (const std::exception &e) { std::printf("    threw: %s\n", e.what()); g_failed++; } } while (0)

static OptimizedDataFrame test_df() {                    // create_test_df, functions.rs:4327-4355
    OptimizedDataFrame df;
    df.add_column("a", Float64Column({1.0, 2.0, 3.0, 4.0, 5.0}));
    df.add_column("b", Float64Column({5.0, 4.0, 3.0, 2.0, 1.0}));
    df.add_column("name", StringColumn({"Alice", "Bob", "Charlie", "David", "Eve"}));
    df.add_column("flag", BooleanColumn({true, false, true, false, true}));
    return df;
}

static OptimizedDataFrame one_column(const std::vector<double> &v) {
    OptimizedDataFrame df;
    df.add_column("a", Float64Column(v));
    return df;
}

template <class F>
static void expect_kind(F &&f, Error::Kind kind, int line) {
    try { f(); std::printf("    no throw (line %d)\n", line); g_failed++; }
    catch (const Error &e) { if (e.kind != kind) { std::printf("    wrong kind (line %d): %s\n", line, e.what()); g_failed++; } }
}

static void test_errors_before_any_device_call() {
    auto df = test_df();
    const auto each = [&](const std::string &c) {
        return std::vector<std::function<void()>>{
            [&df, c] { df.skew(c); }, [&df, c] { df.kurtosis(c); }, [&df, c] { df.sem(c); }, [&df, c] { df.mad(c); }, [&df, c] { df.prod(c); },
            [&df, c] { df.var_column(c); }, [&df, c] { df.std_column(c); }, [&df, c] { df.range(c); }, [&df, c] { df.abs_sum(c); },
            [&df, c] { df.cv(c); }, [&df, c] { df.geometric_mean(c); }, [&df, c] { df.harmonic_mean(c); }, [&df, c] { df.iqr(c); },
            [&df, c] { df.percentile_value(c, 0.5); }, [&df, c] { df.trimmed_mean(c, 0.1); }, [&df, c] { df.describe_column(c); },
            [&df, c] { df.zscore(c); }};
    };
    for (auto &f : each("nope")) expect_kind(f, Error::ColumnNotFound, __LINE__);
    for (auto &f : each("name")) expect_kind(f, Error::Type, __LINE__);
    for (auto &f : each("flag")) expect_kind(f, Error::Type, __LINE__);
    // the reference's early returns for the argument come before any device call too (aggregations.rs:185, :204)
    CHECK(std::isnan(df.percentile_value("a", -0.1)) && std::isnan(df.percentile_value("a", 1.5)));
    CHECK(std::isnan(df.trimmed_mean("a", 0.5)) && std::isnan(df.trimmed_mean("a", -0.01)));
    CHECK(PANDRS_HIP_MOMENTS_WANT_CENTRAL == 1 && PANDRS_HIP_MOMENTS_WANT_LOG == 2 && PANDRS_HIP_MOMENTS_WANT_RECIP == 4 &&
          PANDRS_HIP_MOMENTS_WANT_PROD == 8 && PANDRS_HIP_MOMENTS_MAX_COLUMNS == 16 && PANDRS_HIP_OS_TRIMMED_MEAN == 3);
    CHECK(sizeof(pandrs_hip_moments_stats) == 15 * 8);
}

static bool near(double a, double b, double tol) { return std::fabs(a - b) < tol; }

static void test_column_statistics() {
    for (int resident = 0; resident < 2; resident++) {
        auto df = test_df();
        if (resident) df.make_resident();
        CHECK(near(df.skew("a"), 0.0, 0.1));                                    // test_skew
        CHECK(!std::isnan(df.kurtosis("a")));                                   // test_kurtosis
        {   // the reference's expression on this column's exact sums (m2 = 10, m4 = 34): the same operations, so the same bits
            const double sd = std::sqrt(10.0 / 5.0), k = (34.0 / 5.0) / ((sd * sd) * (sd * sd)) - 3.0;
            CHECK(df.kurtosis("a") == ((5.0 - 1.0) / ((5.0 - 2.0) * (5.0 - 3.0))) * ((5.0 + 1.0) * k + 6.0));
        }
        CHECK(df.var_column("a", 0) == 2.0);                                    // test_var_column
        CHECK(near(df.std_column("a", 0), std::sqrt(2.0), 0.0001));             // test_std_column
        CHECK(near(df.sem("a", 1), 0.707, 0.01));                               // test_sem
        CHECK(near(df.mad("a"), 1.2, 0.0001));                                  // test_mad
        CHECK(df.iqr("a") == 2.0);                                              // test_iqr: sorted[3] - sorted[1]
        CHECK(df.percentile_value("a", 0.0) == 1.0 && df.percentile_value("a", 1.0) == 5.0 && df.percentile_value("a", 0.5) == 3.0);
        const auto d = df.describe_column("a");                                 // test_describe_column
        CHECK(d.at("count") == 5.0 && d.at("mean") == 3.0 && d.at("min") == 1.0 && d.at("max") == 5.0 && d.at("25%") == 2.0 &&
              d.at("50%") == 3.0 && d.at("75%") == 4.0 && d.at("std") == std::sqrt(2.5));
        const auto z = df.zscore("a");                                          // test_zscore
        CHECK(z.size() == 5 && z[0] < 0.0 && std::fabs(z[2]) < 0.001 && z[4] > 0.0);
    }
    CHECK(std::isnan(one_column({1.0, 2.0}).skew("a")));                        // test_skew_insufficient_data
    CHECK(std::isnan(one_column({1.0, 2.0, 3.0}).kurtosis("a")));               // test_kurtosis_insufficient_data
    expect_kind([] { one_column({1.0}).zscore("a"); }, Error::InvalidValue, __LINE__);     // test_zscore_insufficient_values
    expect_kind([] { one_column({4.0, 4.0, 4.0}).zscore("a"); }, Error::InvalidValue, __LINE__);
    CHECK(one_column({1.0, 2.0, 3.0, 4.0}).prod("a") == 24.0);                  // test_prod
    CHECK(one_column({-2.0, 1.0, 5.0}).range("a") == 7.0 && one_column({-2.0, 1.0, 5.0}).abs_sum("a") == 8.0);      // test_range_abs_sum
    CHECK(near(one_column({1.0, 2.0, 4.0, 8.0}).geometric_mean("a"), 2.828, 0.01));        // test_geometric_mean
    CHECK(near(one_column({1.0, 2.0, 4.0}).harmonic_mean("a"), 1.714, 0.01));   // test_harmonic_mean
    CHECK(one_column({1.0, 2.0, 4.0}).harmonic_mean("a") == 3.0 / 1.75);
    const double cv = one_column({10.0, 20.0, 30.0}).cv("a");                   // test_cv
    CHECK(cv > 0.0 && cv < 1.0);
    CHECK(near(one_column({1.0, 2.0, 3.0, 4.0, 100.0}).trimmed_mean("a", 0.2), 3.0, 0.1));  // test_trimmed_mean
    CHECK(one_column({1.0, 1.0, 1.0, 2.0, 3.0, 3.0, 3.0, 3.0}).trimmed_mean("a", 0.25) == 2.25);        // ties at both cuts
    // no valid cell
    const auto none = one_column({NAN, NAN});
    CHECK(std::isnan(none.mad("a")) && std::isnan(none.prod("a")) && std::isnan(none.range("a")) && std::isnan(none.cv("a")) &&
          std::isnan(none.iqr("a")) && std::isnan(none.percentile_value("a", 0.5)) && std::isnan(none.trimmed_mean("a", 0.1)));
    CHECK(none.describe_column("a").size() == 5 && none.describe_column("a").at("count") == 0.0);
}

static void test_frame_lists() {
    OptimizedDataFrame df;
    df.add_column("a", Float64Column({1.0, 2.0, 3.0}));
    df.add_column("s", StringColumn({"x", "y", "z"}));
    df.add_column("b", Float64Column({10.0, 20.0, 30.0}));
    df.add_column("n", Float64Column({NAN, NAN, NAN}));
    df.add_column("i", Int64Column({4, 1, 7}));
    using NV = OptimizedDataFrame::NamedValues;
    CHECK((df.sum_all() == NV{{"a", 6.0}, {"b", 60.0}, {"n", 0.0}, {"i", 12.0}}));                        // test_sum_all
    CHECK((df.mean_all() == NV{{"a", 2.0}, {"b", 20.0}, {"i", 4.0}}));                                     // test_mean_all
    CHECK((df.min_all() == NV{{"a", 1.0}, {"b", 10.0}, {"i", 1.0}}));
    CHECK((df.max_all() == NV{{"a", 3.0}, {"b", 30.0}, {"i", 7.0}}));
    CHECK((df.var_all() == NV{{"a", 1.0}, {"b", 100.0}, {"i", 9.0}}));
    CHECK((df.std_all() == NV{{"a", 1.0}, {"b", 10.0}, {"i", 3.0}}));
    CHECK((df.product_all() == NV{{"a", 6.0}, {"b", 6000.0}, {"i", 28.0}}));
    CHECK((df.median_all() == NV{{"a", 2.0}, {"b", 20.0}, {"i", 4.0}}));
    CHECK((one_column({1.0, 2.0, 3.0, 4.0}).median_all() == NV{{"a", 2.5}}));                              // test_median_all_even
    CHECK((one_column({2.0, NAN, 3.0}).product_all() == NV{{"a", 6.0}}));                                  // test_product_all_with_nan
    CHECK((one_column({1.0, 2.0, 3.0, 4.0, 5.0}).var_all() == NV{{"a", 2.5}}));                            // test_var_all
}

int main() {
    RUN(test_errors_before_any_device_call);
    int32_t n_dev = 0;
    if (pandrs_hip_init(nullptr) != PANDRS_HIP_OK || pandrs_hip_device_count(&n_dev) != PANDRS_HIP_OK || n_dev == 0) {
        std::printf("%d tests, %d failed checks\n", g_run, g_failed);
        std::fprintf(stderr, "no HIP device available: %s\n", pandrs_hip_last_error());
        return g_failed ? 2 : 1;
    }
    RUN(test_column_statistics);
    RUN(test_frame_lists);
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
