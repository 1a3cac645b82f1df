// PandasCompatExt's row masks (gt / ge / lt / le / eq_value / ne_value, between / is_between, isna / notna, is_finite /
// is_infinite, isin / isin_numeric, query_gt / query_lt / query_eq, dropna, count_na, has_nulls, count_value) through the C++ host
// mirror (include/pandrs_hip.hpp) over libpandrs_hip.so: the reference's known answers (src/dataframe/pandas_compat/functions.rs:
// 4362-4367, :4405-4410, :4988-4993, :5007-5008, :7264-7268, :8121-8147, :8206, :8348-8352, :8483-8485, :8520-8524, :8632-8633).
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "pandrs_hip.hpp"

using namespace pandrs;

static int g_failed = 0, g_run = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("    CHECK failed: %s  (%s:%d)\n", #cond, __FILE__, __LINE__); g_failed++; } } while (0)
#define RUN(fn) do { g_run++; std::printf("test %s\n", #fn); try { fn(); } catch (const std::exception &e) { std::printf("    threw: %s\n", e.what()); g_failed++; } } while (0)

using B = std::vector<bool>;

static OptimizedDataFrame test_df() {                    // create_test_df, functions.rs:4327-4355
    OptimizedDataFrame df;
    df.add_column("a", Float64Column({1.0, 2.0, 3.0, 4.0, 5.0}));
    df.add_column("b", Float64Column({5.0, 4.0, 3.0, 2.0, 1.0}));
    df.add_column("name", StringColumn({"Alice", "Bob", "Charlie", "David", "Eve"}));
    df.add_column("flag", BooleanColumn({true, false, true, false, true}));
    return df;
}

static void test_errors_before_any_device_call() {
    auto df = test_df();
    try { df.gt("nope", 1.0); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.between("name", 1.0, 2.0); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.isna("flag"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type && std::string(e.what()) == "Column 'flag' is not a numeric type"); }
    try { df.count_na("name"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.query_gt("flag", 0.0); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.dropna("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.isin("a", {"x"}); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.isin_numeric("name", {1.0}); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    OptimizedDataFrame empty;
    empty.add_column("v", Float64Column(std::vector<double>{}));
    CHECK(empty.gt("v", 0.0).empty() && empty.count_na("v") == 0 && !empty.has_nulls("v") && empty.isin_numeric("v", {1.0}).empty());
    CHECK(empty.dropna("v").row_count() == 0 && empty.dropna("v").column_count() == 1);
    CHECK(PANDRS_HIP_PRED_GT == 0 && PANDRS_HIP_PRED_NE == 5 && PANDRS_HIP_PRED_BETWEEN == 6 && PANDRS_HIP_PRED_BETWEEN_EXCLUSIVE == 7 &&
          PANDRS_HIP_PRED_ISNA == 8 && PANDRS_HIP_PRED_IS_INFINITE == 11);
}

static void test_known_answers() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int resident = 0; resident < 2; resident++) {
        auto df = test_df();
        OptimizedDataFrame na;
        na.add_column("a", Float64Column({1.0, nan, 3.0, nan, 5.0}));
        na.add_column("b", Float64Column({10.0, 20.0, 30.0, 40.0, 50.0}));
        na.add_column("i", Int64Column::with_nulls({7, 8, 9, 10, 11}, {false, false, true, false, false}));
        if (resident) { df.make_resident(); na.make_resident(); }
        CHECK((df.between("a", 2.0, 4.0) == B{false, true, true, true, false}));                 // functions.rs:4405-4410
        CHECK((df.gt("a", 3.0) == B{false, false, false, true, true}));                           // :8121-8131
        CHECK((df.ge("a", 3.0) == B{false, false, true, true, true}));
        CHECK((df.lt("a", 3.0) == B{true, true, false, false, false}));
        CHECK((df.le("a", 3.0) == B{true, true, true, false, false}));
        CHECK((df.is_between("a", 2.0, 4.0, true) == B{false, true, true, true, false}));        // :8520-8524
        CHECK((df.is_between("a", 2.0, 4.0, false) == B{false, false, true, false, false}));
        CHECK((df.eq_value("b", 2.0) == B{false, false, false, true, false}));
        CHECK((df.ne_value("b", 2.0) == B{true, true, true, false, true}));
        CHECK((df.isin("name", {"Alice", "Bob", "Unknown-to-this-pool"}) == B{true, true, false, false, false}));   // :4362-4367
        CHECK((df.isin_numeric("a", {2.0, 5.0, -0.0}) == B{false, true, false, false, true}));
        const auto q = df.query_gt("a", 3.0);                                                     // :7264-7268
        CHECK(q.row_count() == 2 && q.column_count() == 4);
        CHECK((std::get<Float64Column>(q.column("a")).data == std::vector<double>{4.0, 5.0}));
        CHECK((std::get<Float64Column>(q.column("b")).data == std::vector<double>{2.0, 1.0}));
        CHECK(df.query_lt("a", 3.0).row_count() == 2 && df.query_eq("a", 3.0).row_count() == 1 && df.query_gt("a", 9.0).row_count() == 0);
        CHECK((na.isna("a") == B{false, true, false, true, false}));                              // :5007-5008
        CHECK((na.notna("a") == B{true, false, true, false, true}));
        CHECK(na.count_na("a") == 2 && na.has_nulls("a") && !na.has_nulls("b") && na.count_value("b", 30.0) == 1);
        CHECK((na.isna("i") == B{false, false, true, false, false}) && (na.gt("i", 7.5) == B{false, true, false, true, true}));   // a null cell is NaN
        const auto d = na.dropna("a");                                                            // :4988-4993
        CHECK(d.row_count() == 3);
        CHECK((std::get<Float64Column>(d.column("a")).data == std::vector<double>{1.0, 3.0, 5.0}));
        CHECK((std::get<Float64Column>(d.column("b")).data == std::vector<double>{10.0, 30.0, 50.0}));
    }
    OptimizedDataFrame fin;
    fin.add_column("a", Float64Column({1.0, inf, -inf, nan}));
    CHECK((fin.is_finite("a") == B{true, false, false, false}) && (fin.is_infinite("a") == B{false, true, true, false}));   // :8348-8352
    CHECK((fin.eq_value("a", inf) == B{false, false, false, false}) && (fin.ne_value("a", inf) == B{true, false, true, true}));
    // the C ABI: a guarded output at an odd offset, the count-only form and an unknown op
    const std::vector<double> x = {3.0, 1.0, 4.0, 1.0, 5.0, 9.0, 2.0, 6.0, 5.0, 3.0};
    const pandrs_hip_column col{x.data(), nullptr, PANDRS_HIP_F64, 0};
    uint8_t out[5] = {0xAA, 0xAA, 0xAA, 0xAA, 0xAA};
    int64_t count = -1;
    CHECK(pandrs_hip_predicate(detail::context(), PANDRS_HIP_MEM_HOST, &col, 10, 12, 0.0, 0.0, PANDRS_HIP_MEM_HOST, out + 1, &count) == PANDRS_HIP_ERR_INVALID_ARGUMENT);
    CHECK(pandrs_hip_predicate(detail::context(), PANDRS_HIP_MEM_HOST, &col, 10, PANDRS_HIP_PRED_GE, 4.0, 0.0, PANDRS_HIP_MEM_HOST, out + 1, &count) == PANDRS_HIP_OK);
    CHECK(count == 5 && out[0] == 0xAA && out[1] == 0xB4 && out[2] == 0x01 && out[3] == 0xAA);
    count = -1;
    CHECK(pandrs_hip_predicate(detail::context(), PANDRS_HIP_MEM_HOST, &col, 10, PANDRS_HIP_PRED_LT, 4.0, 0.0, PANDRS_HIP_MEM_HOST, nullptr, &count) == PANDRS_HIP_OK && count == 5);
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
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
