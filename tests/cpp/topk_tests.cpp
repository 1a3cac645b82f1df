// PandasCompatExt::nlargest / nsmallest / idxmax / idxmin (src/dataframe/pandas_compat/functions.rs:159-192) through the C++
// host mirror (include/pandrs_hip.hpp) over libpandrs_hip.so: the reference's known answers (functions.rs:4369-4391) and two
// tie cases (ties in row order; the first minimum and the last maximum).
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

static OptimizedDataFrame tie_frame() {
    OptimizedDataFrame df;
    df.add_column("i", Int64Column({4, 1, 4, 1, 5, 4, 4}));
    df.add_column("gaps", Float64Column::with_nulls({2.0, NAN, 0.0, 7.0, -0.0, 2.0, -1.0}, {false, false, false, true, false, false, false}));
    df.add_column("row", Int64Column({0, 1, 2, 3, 4, 5, 6}));
    return df;
}

static std::vector<int64_t> rows_of(const OptimizedDataFrame &df) { return std::get<Int64Column>(df.column("row")).data; }

static void test_errors_before_any_device_call() {
    auto df = test_df();
    try { df.nlargest(2, "nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.nsmallest(2, "name"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.idxmax("flag"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type && std::string(e.what()) == "Column 'flag' is not a numeric type"); }
    try { df.idxmin("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    CHECK(df.nlargest(0, "a").row_count() == 0 && df.nlargest(0, "a").column_count() == 0);
    OptimizedDataFrame empty;
    empty.add_column("v", Float64Column(std::vector<double>{}));
    CHECK(empty.nsmallest(3, "v").column_count() == 0 && !empty.idxmax("v").has_value() && !empty.idxmin("v").has_value());
    CHECK(PANDRS_HIP_TOPK_LARGEST == 0 && PANDRS_HIP_TOPK_SMALLEST == 1);
}

static void test_known_answers() {
    for (int resident = 0; resident < 2; resident++) {
        auto df = test_df();
        auto tf = tie_frame();
        if (resident) { df.make_resident(); tf.make_resident(); }
        const auto top = df.nlargest(3, "a");                                       // functions.rs:4369-4373
        CHECK(top.row_count() == 3 && top.column_count() == 4);
        CHECK((std::get<Float64Column>(top.column("a")).data == std::vector<double>{5.0, 4.0, 3.0}));
        CHECK((std::get<Float64Column>(top.column("b")).data == std::vector<double>{1.0, 2.0, 3.0}));
        const auto low = df.nsmallest(2, "a");                                      // :4375-4379
        CHECK(low.row_count() == 2 && (std::get<Float64Column>(low.column("a")).data == std::vector<double>{1.0, 2.0}));
        CHECK(df.nlargest(9, "a").row_count() == 5);
        CHECK(df.idxmax("a") == std::optional<size_t>(4) && df.idxmin("a") == std::optional<size_t>(0));   // :4381-4391
        CHECK(df.idxmax("b") == std::optional<size_t>(0) && df.idxmin("b") == std::optional<size_t>(4));
        // ties in row order; the quota ends inside the run of 4s
        CHECK((rows_of(tf.nlargest(3, "i")) == std::vector<int64_t>{4, 0, 2}));
        CHECK((rows_of(tf.nsmallest(4, "i")) == std::vector<int64_t>{1, 3, 0, 2}));
        CHECK(tf.idxmax("i") == std::optional<size_t>(4) && tf.idxmin("i") == std::optional<size_t>(1));
        // -0.0 ties 0.0, NaN after every number, the null row last, in both directions
        CHECK((rows_of(tf.nlargest(7, "gaps")) == std::vector<int64_t>{0, 5, 2, 4, 6, 1, 3}));
        CHECK((rows_of(tf.nsmallest(7, "gaps")) == std::vector<int64_t>{6, 2, 4, 0, 5, 1, 3}));
        CHECK(tf.idxmax("gaps") == std::optional<size_t>(5) && tf.idxmin("gaps") == std::optional<size_t>(6));
    }
    const std::vector<double> x = {3.0, 1.0, 4.0, 1.0, 5.0};
    const pandrs_hip_column col{x.data(), nullptr, PANDRS_HIP_F64, 0};
    int64_t out[6] = {-7, -7, -7, -7, -7, -7}, count = 0, numbers = 0;
    CHECK(pandrs_hip_topk(detail::context(), PANDRS_HIP_MEM_HOST, &col, 5, 2, 2, PANDRS_HIP_MEM_HOST, out, &count, &numbers) == PANDRS_HIP_ERR_INVALID_ARGUMENT);
    CHECK(pandrs_hip_topk(detail::context(), PANDRS_HIP_MEM_HOST, &col, 5, 2, PANDRS_HIP_TOPK_SMALLEST, PANDRS_HIP_MEM_HOST, out, &count, &numbers) == PANDRS_HIP_OK);
    CHECK(count == 2 && numbers == 2 && out[0] == 1 && out[1] == 3 && out[2] == -7);
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
