// PandasCompatExt::value_range / cut / qcut (src/dataframe/pandas_compat/functions.rs:2270-2282, :2339-2420) through the C++
// host mirror (include/pandrs_hip.hpp) over libpandrs_hip.so: the reference's tests test_value_range (functions.rs:6840-6846),
// test_cut, test_cut_with_nan, test_cut_zero_bins, test_qcut, test_qcut_with_nan, test_qcut_zero_quantiles (:6943-7018), with
// the full label lists the reference's loops give for those inputs.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "pandrs_hip.hpp"

using namespace pandrs;

static int g_failed = 0, g_run = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("    CHECK failed: %s  (%s:%d)\n", #cond, __FILE__, __LINE__); g_failed++; } } while (0)
#define RUN(fn) do { g_run++; std::printf("test %s\n", #fn); try { fn(); } catch (const std::exception &e) { std::printf("    threw: %s\n", e.what()); g_failed++; } } while (0)

using Strings = std::vector<std::string>;

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

static void test_errors_before_any_device_call() {
    auto df = test_df();
    try { df.cut("nope", 2); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.qcut("nope", 2); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.value_range("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.cut("name", 2); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.qcut("flag", 2); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type && std::string(e.what()) == "Column 'flag' is not a numeric type"); }
    try { df.value_range("name"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    // test_cut_zero_bins (:6973-6977), test_qcut_zero_quantiles (:7013-7018)
    try { df.cut("a", 0); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue && std::string(e.what()) == "Number of bins must be > 0"); }
    try { df.qcut("a", 0); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue && std::string(e.what()) == "Number of quantiles must be > 0"); }
    try { df.cut("a", PANDRS_HIP_BIN_MAX_BINS + 1); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    OptimizedDataFrame empty;
    empty.add_column("v", Float64Column(std::vector<double>{}));
    try { empty.cut("v", 2); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue && std::string(e.what()) == "No valid values in column"); }
    try { empty.qcut("v", 2); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue && std::string(e.what()) == "No valid values"); }
    try { empty.value_range("v"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    CHECK(PANDRS_HIP_BIN_CUT == 0 && PANDRS_HIP_BIN_QCUT == 1 && PANDRS_HIP_BIN_NONE == -1 && PANDRS_HIP_BIN_NAN == -2);
}

static void test_value_range() {                         // :6840-6846
    const auto r = test_df().value_range("a");
    CHECK(r.first == 1.0 && r.second == 5.0);
    const auto s = one_column({NAN, 2.0, -7.5, NAN}).value_range("a");
    CHECK(s.first == -7.5 && s.second == 2.0);
    try { one_column({NAN, NAN}).value_range("a"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
}

static void test_cut() {                                 // :6943-6956
    for (int resident = 0; resident < 2; resident++) {
        auto df = one_column({1.0, 2.5, 4.0, 5.0});
        if (resident) df.make_resident();
        const Strings got = df.cut("a", 2);
        CHECK(got.size() == 4);
        CHECK((got == Strings{"(1.00, 3.00]", "(1.00, 3.00]", "(3.00, 5.00]", "(3.00, 5.00]"}));
    }
    // the maximum falls out of the last bin once max + 0.001 == max: the result is shorter than the column
    const Strings big = one_column({0.0, 1e15, 5e14}).cut("a", 2);
    CHECK((big == Strings{"(0.00, 500000000000000.00]", "(500000000000000.00, 1000000000000000.00]"}));
    // a width that is not finite: every bin is empty, the NaN rows alone answer
    CHECK((one_column({1.0, NAN, INFINITY}).cut("a", 2) == Strings{"NaN"}));
}

static void test_cut_with_nan() {                        // :6958-6970
    const Strings got = one_column({1.0, NAN, 3.0}).cut("a", 2);
    CHECK(got.size() == 3 && got[1] == "NaN");
    CHECK((got == Strings{"(1.00, 2.00]", "NaN", "(2.00, 3.00]"}));
    try { one_column({NAN}).cut("a", 2); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
}

static void test_qcut() {                                // :6979-6997
    for (int resident = 0; resident < 2; resident++) {
        auto df = one_column({1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0});
        if (resident) df.make_resident();
        const Strings got = df.qcut("a", 4);
        CHECK(got.size() == 8);
        CHECK((got == Strings{"Q1", "Q1", "Q2", "Q2", "Q3", "Q3", "Q4", "Q4"}));
    }
    OptimizedDataFrame ints;
    ints.add_column("a", Int64Column({5, 1, 3, 3, 9}));
    CHECK((ints.qcut("a", 2) == Strings{"Q2", "Q1", "Q2", "Q2", "Q2"}));     // edges 1, 3, 9
}

static void test_qcut_with_nan() {                       // :6999-7011
    const Strings got = one_column({1.0, NAN, 3.0, 4.0}).qcut("a", 2);
    CHECK(got.size() == 4 && got[1] == "NaN");
    CHECK((got == Strings{"Q1", "NaN", "Q2", "Q2"}));                         // edges 1, 3, 4
    try { one_column({NAN, NAN}).qcut("a", 2); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
}

int main() {
    RUN(test_errors_before_any_device_call);
    int32_t n_dev = 0;
    if (pandrs_hip_init(nullptr) != PANDRS_HIP_OK || pandrs_hip_device_count(&n_dev) != PANDRS_HIP_OK || n_dev == 0) {
        std::printf("%d tests, %d failed checks\n", g_run, g_failed);
        std::fprintf(stderr, "no HIP device available: %s\n", pandrs_hip_last_error());
        return g_failed ? 2 : 1;
    }
    RUN(test_value_range);
    RUN(test_cut);
    RUN(test_cut_with_nan);
    RUN(test_qcut);
    RUN(test_qcut_with_nan);
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
