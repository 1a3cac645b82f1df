// OptimizedDataFrame::describe / describe_all (src/optimized/split_dataframe/stats.rs:50-171 over
// src/stats/descriptive.rs:91-200) through the C++ host mirror (include/pandrs_hip.hpp) over libpandrs_hip.so: the
// reference's known answers (descriptive.rs:612-632, stats.rs:567-583, tests/stats_comprehensive_test.rs:478-487).
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
    df.add_column("values", Float64Column({1.0, 2.0, 3.0, 4.0, 5.0}));
    df.add_column("i", Int64Column({5, 1, 4, 2, 3}));
    df.add_column("constant", Float64Column({5.0, 5.0, 5.0, 5.0, 5.0}));
    df.add_column("nothing", Float64Column::with_nulls({1.0, 2.0, 3.0, 4.0, 5.0}, {true, true, true, true, true}));
    df.add_column("s", StringColumn({"a", "b", "c", "d", "e"}));
    df.add_column("b", BooleanColumn({true, false, true, false, true}));
    return df;
}

static void test_errors_before_any_device_call() {
    auto df = sample_frame();
    try { df.describe("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.describe("s"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.describe("b"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type && std::string(e.what()) == "Column 'b' is not a numeric type"); }
    OptimizedDataFrame empty;
    empty.add_column("v", Float64Column(std::vector<double>{}));
    try { empty.describe("v"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    CHECK(empty.describe_all().empty());
    CHECK(sizeof(pandrs_hip_describe_stats) == 64);
}

static void test_known_answers() {
    for (int resident = 0; resident < 2; resident++) {
        auto df = sample_frame();
        if (resident) df.make_resident();
        for (const char *name : {"values", "i"}) {
            const StatDescribe d = df.describe(name);
            const std::vector<std::string> order = {"count", "mean", "std", "min", "25%", "50%", "75%", "max"};
            CHECK(d.stats_list.size() == 8 && d.stats.size() == 8);
            for (size_t k = 0; k < order.size() && k < d.stats_list.size(); k++)
                CHECK(d.stats_list[k].first == order[k] && d.stats.at(order[k]) == d.stats_list[k].second);
            CHECK(d.stats.at("count") == 5.0 && d.stats.at("mean") == 3.0 && d.stats.at("50%") == 3.0);
            CHECK(d.stats.at("min") == 1.0 && d.stats.at("max") == 5.0 && d.stats.at("25%") == 2.0 && d.stats.at("75%") == 4.0);
            CHECK(std::fabs(d.stats.at("std") - std::sqrt(2.5)) <= 1e-9 * std::sqrt(2.5));
        }
        const StatDescribe c = df.describe("constant");
        CHECK(c.stats.at("std") == 0.0 && c.stats.at("min") == 5.0 && c.stats.at("50%") == 5.0 && c.stats.at("max") == 5.0);
        try { df.describe("nothing"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
        const auto all = df.describe_all();
        CHECK(all.size() == 3 && all.count("values") && all.count("i") && all.count("constant") && !all.count("nothing"));
    }
    // percentile's edges through the C ABI (descriptive.rs:625-632, stats_comprehensive_test.rs:484-487)
    const std::vector<double> x = {1.0, 2.0, 3.0, 4.0, 5.0};
    const pandrs_hip_column col{x.data(), nullptr, PANDRS_HIP_F64, 0};
    const double ps[3] = {0.0, 50.0, 100.0};
    double out[3] = {0, 0, 0};
    int64_t count = 0;
    CHECK(pandrs_hip_quantiles(detail::context(), PANDRS_HIP_MEM_HOST, &col, 5, ps, 3, out, &count) == PANDRS_HIP_OK);
    CHECK(count == 5 && out[0] == 1.0 && out[1] == 3.0 && out[2] == 5.0);
    for (double bad : {-1.0, 101.0})
        CHECK(pandrs_hip_quantiles(detail::context(), PANDRS_HIP_MEM_HOST, &col, 5, &bad, 1, out, &count) == PANDRS_HIP_ERR_INVALID_ARGUMENT);
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
