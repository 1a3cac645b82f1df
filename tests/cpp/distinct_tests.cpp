// PandasCompatExt::value_counts / unique / nunique / mode_* / is_unique (src/dataframe/pandas_compat/functions.rs:343-384,
// :775-788, :1709-1753, :4120-4139, :4226-4259) through the C++ host mirror (include/pandrs_hip.hpp) over libpandrs_hip.so: the
// reference's tests test_nunique (:4449), test_value_counts (:4471), test_value_counts_numeric (:4495), test_unique (:4715),
// test_unique_numeric (:4739), test_mode_numeric / _multiple / test_mode_string (:6012-6057), test_nunique_all (:8503),
// test_is_unique (:8667), test_mode_with_count (:8685), with the full lists the reference's loops give for those inputs.
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
using StringCounts = std::vector<std::pair<std::string, size_t>>;
using NumberCounts = std::vector<std::pair<double, size_t>>;

static OptimizedDataFrame test_df() {                    // create_test_df, functions.rs:4327-4355
    OptimizedDataFrame df;
    df.add_column("a", Float64Column({1.0, 2.0, 3.0, 4.0, 5.0}));
    df.add_column("b", Float64Column({5.0, 4.0, 3.0, 2.0, 1.0}));
    df.add_column("name", StringColumn({"Alice", "Bob", "Charlie", "David", "Eve"}));
    return df;
}

static OptimizedDataFrame numbers(const std::vector<double> &v) {
    OptimizedDataFrame df;
    df.add_column("a", Float64Column(v));
    return df;
}

static OptimizedDataFrame strings(const Strings &v) {
    OptimizedDataFrame df;
    df.add_column("cat", StringColumn(v));
    return df;
}

static void test_errors_before_any_device_call() {
    auto df = test_df();
    df.add_column("flag", BooleanColumn({true, false, true, false, true}));
    try { df.value_counts("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.value_counts_numeric("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.unique("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.unique_numeric("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.mode_numeric("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.mode_string("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.mode_with_count("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.is_unique("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.value_counts_numeric("name"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type && std::string(e.what()) == "Column 'name' is not a numeric type"); }
    try { df.unique_numeric("flag"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.mode_numeric("name"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.mode_with_count("flag"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.mode_string("a"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type && std::string(e.what()) == "Column 'a' is not a string type"); }
    // no rows: empty lists without a device call
    OptimizedDataFrame empty;
    empty.add_column("a", Float64Column(std::vector<double>{}));
    CHECK(empty.value_counts_numeric("a").empty() && empty.unique_numeric("a").empty() && empty.mode_numeric("a").empty());
    CHECK(empty.value_counts("a").empty() && empty.unique("a").empty() && empty.is_unique("a"));
    const auto m = empty.mode_with_count("a");
    CHECK(m.first != m.first && m.second == 0);
    CHECK(empty.nunique() == (StringCounts{{"a", 0}}) && empty.nunique_all().at("a") == 0);
    CHECK(PANDRS_HIP_DISTINCT_BY_VALUE == 0 && PANDRS_HIP_DISTINCT_BY_COUNT == 1);
}

static void test_nunique() {                             // :4449-4455
    const auto r = test_df().nunique();
    CHECK(r.size() == 3);
    for (auto &e : r) CHECK(e.second == 5);
    CHECK(r[0].first == "a" && r[2].first == "name");
}

static void test_value_counts() {                        // :4471-4493, tests/categorical_df_test.rs:82-112
    const auto c = strings({"A", "B", "A", "C", "A"}).value_counts("cat");
    CHECK((c == StringCounts{{"A", 3}, {"B", 1}, {"C", 1}}));
    const auto t = strings({"Tokyo", "Osaka", "Tokyo", "Nagoya", "Osaka"}).value_counts("cat");
    CHECK((t == StringCounts{{"Osaka", 2}, {"Tokyo", 2}, {"Nagoya", 1}}));
    // a numeric column is stringified first (get_column_string_values), ties by string
    CHECK((numbers({10.0, 9.0, 10.0, 2.5}).value_counts("a") == StringCounts{{"10", 2}, {"2.5", 1}, {"9", 1}}));
}

static void test_value_counts_numeric() {                // :4495-4502
    const auto r = test_df().value_counts_numeric("a");
    CHECK((r == NumberCounts{{1.0, 1}, {2.0, 1}, {3.0, 1}, {4.0, 1}, {5.0, 1}}));
    const auto n = numbers({2.0, NAN, 1.0, 2.0, NAN, 7.5}).value_counts_numeric("a");
    CHECK(n.size() == 4 && n[0] == (std::pair<double, size_t>{2.0, 2}) && n[1].first != n[1].first && n[1].second == 2);
    CHECK(n[2] == (std::pair<double, size_t>{1.0, 1}) && n[3] == (std::pair<double, size_t>{7.5, 1}));
}

static void test_unique() {                              // :4715-4737
    CHECK((strings({"A", "B", "A", "C", "A"}).unique("cat") == Strings{"A", "B", "C"}));
}

static void test_unique_numeric() {                      // :4739-4749
    CHECK((numbers({1.0, 2.0, 1.0, 3.0, 2.0, 1.0}).unique_numeric("a") == std::vector<double>{1.0, 2.0, 3.0}));
    const auto z = numbers({0.0, -0.0, -1.0}).unique_numeric("a");
    CHECK(z.size() == 3 && z[0] == -1.0 && std::signbit(z[1]) && !std::signbit(z[2]));
}

static void test_mode_numeric() {                        // :6012-6035
    CHECK((numbers({1.0, 2.0, 2.0, 3.0, 3.0, 3.0}).mode_numeric("a") == std::vector<double>{3.0}));
    CHECK((numbers({1.0, 1.0, 2.0, 2.0, 3.0}).mode_numeric("a") == std::vector<double>{1.0, 2.0}));
    CHECK(numbers({NAN, NAN}).mode_numeric("a").empty());
}

static void test_mode_string() {                         // :6038-6057
    CHECK((strings({"a", "b", "a", "c"}).mode_string("cat") == Strings{"a"}));
    CHECK((strings({"", "", "", "b", "a"}).mode_string("cat") == Strings{"a", "b"}));
}

static void test_nunique_all() {                         // :8503-8509
    const auto r = test_df().nunique_all();
    CHECK(r.at("a") == 5 && r.at("name") == 5 && r.at("b") == 5);
    CHECK(numbers({1.0, NAN, 1.0, 2.0}).nunique_all().at("a") == 2);
}

static void test_is_unique() {                           // :8667-8682
    CHECK(numbers({1.0, 2.0, 3.0}).is_unique("a"));
    CHECK(!numbers({1.0, 1.0, 2.0}).is_unique("a"));
    CHECK(numbers({1.0, NAN, NAN, 2.0}).is_unique("a"));
}

static void test_mode_with_count() {                     // :8685-8696
    const auto m = numbers({1.0, 2.0, 2.0, 3.0, 2.0}).mode_with_count("a");
    CHECK(m.first == 2.0 && m.second == 3);
    const auto t = numbers({5.0, 4.0, 5.0, 4.0}).mode_with_count("a");              // a tie: the smallest
    CHECK(t.first == 4.0 && t.second == 2);
    const auto n = numbers({NAN}).mode_with_count("a");
    CHECK(n.first != n.first && n.second == 0);
}

static void test_int_and_null_columns() {
    OptimizedDataFrame df;
    df.add_column("i", Int64Column::with_nulls({7, 7, -3, 9, 9}, {false, false, false, true, false}));
    df.add_column("s", StringColumn::with_nulls({"x", "y", "x", "y", "y"}, {false, true, false, false, false}));
    const auto v = df.value_counts_numeric("i");
    CHECK(v.size() == 4 && v[0] == (std::pair<double, size_t>{7.0, 2}) && v[1] == (std::pair<double, size_t>{-3.0, 1}));
    CHECK(v[2] == (std::pair<double, size_t>{9.0, 1}) && v[3].first != v[3].first && v[3].second == 1);
    CHECK((df.value_counts("s") == StringCounts{{"x", 2}, {"y", 2}, {"", 1}}));
    CHECK((df.mode_string("s") == Strings{"x", "y"}));
    CHECK(!df.is_unique("i") && df.nunique_all().at("i") == 3 && df.nunique_all().at("s") == 2);
}

int main() {
    RUN(test_errors_before_any_device_call);
    int32_t n_dev = 0;
    if (pandrs_hip_init(nullptr) != PANDRS_HIP_OK || pandrs_hip_device_count(&n_dev) != PANDRS_HIP_OK || n_dev == 0) {
        std::printf("%d tests, %d failed checks\n", g_run, g_failed);
        std::fprintf(stderr, "no HIP device available: %s\n", pandrs_hip_last_error());
        return g_failed ? 2 : 1;
    }
    RUN(test_nunique);
    RUN(test_value_counts);
    RUN(test_value_counts_numeric);
    RUN(test_unique);
    RUN(test_unique_numeric);
    RUN(test_mode_numeric);
    RUN(test_mode_string);
    RUN(test_nunique_all);
    RUN(test_is_unique);
    RUN(test_mode_with_count);
    RUN(test_int_and_null_columns);
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
