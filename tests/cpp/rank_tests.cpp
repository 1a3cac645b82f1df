// PandasCompatExt::rank (src/dataframe/pandas_compat/functions.rs:193-236) through the C++ host mirror
// (include/pandrs_hip.hpp) over libpandrs_hip.so: the reference's known answer (functions.rs:4393-4404) and the five
// methods on [3, 1, 4, 1, 5, 4, 4].
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
    df.add_column("x", Float64Column({3.0, 1.0, 4.0, 1.0, 5.0}));
    df.add_column("s", StringColumn({"a", "b", "c", "d", "e"}));
    df.add_column("b", BooleanColumn({true, false, true, false, true}));
    return df;
}

static OptimizedDataFrame table_frame() {
    OptimizedDataFrame df;
    df.add_column("f", Float64Column({3.0, 1.0, 4.0, 1.0, 5.0, 4.0, 4.0}));
    df.add_column("i", Int64Column({3, 1, 4, 1, 5, 4, 4}));
    df.add_column("gaps", Float64Column::with_nulls({2.0, NAN, 1.0, 7.0, 1.0, 0.0, -0.0}, {false, false, false, true, false, false, false}));
    return df;
}

static void test_errors_before_any_device_call() {
    auto df = sample_frame();
    try { df.rank("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.rank("s"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.rank("b", RankMethod::Dense); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type && std::string(e.what()) == "Column 'b' is not a numeric type"); }
    OptimizedDataFrame empty;
    empty.add_column("v", Float64Column(std::vector<double>{}));
    CHECK(empty.rank("v").empty() && empty.rank("v", RankMethod::First).empty());
    CHECK((int32_t)RankMethod::Average == PANDRS_HIP_RANK_AVERAGE && (int32_t)RankMethod::Min == PANDRS_HIP_RANK_MIN &&
          (int32_t)RankMethod::Max == PANDRS_HIP_RANK_MAX && (int32_t)RankMethod::First == PANDRS_HIP_RANK_FIRST &&
          (int32_t)RankMethod::Dense == PANDRS_HIP_RANK_DENSE);
}

static void test_known_answers() {
    for (int resident = 0; resident < 2; resident++) {
        auto df = sample_frame();
        auto tf = table_frame();
        if (resident) { df.make_resident(); tf.make_resident(); }
        const std::vector<double> ranks = df.rank("x", RankMethod::Average);      // functions.rs:4393-4404
        CHECK(ranks.size() == 5 && ranks[1] == 1.5 && ranks[3] == 1.5 && ranks[0] == 3.0);
        CHECK(df.rank("x") == ranks);
        for (const char *name : {"f", "i"}) {
            CHECK((tf.rank(name, RankMethod::Average) == std::vector<double>{3.0, 1.5, 5.0, 1.5, 7.0, 5.0, 5.0}));
            CHECK((tf.rank(name, RankMethod::Min) == std::vector<double>{3.0, 1.0, 4.0, 1.0, 7.0, 4.0, 4.0}));
            CHECK((tf.rank(name, RankMethod::Max) == std::vector<double>{3.0, 2.0, 6.0, 2.0, 7.0, 6.0, 6.0}));
            CHECK((tf.rank(name, RankMethod::First) == std::vector<double>{3.0, 1.0, 4.0, 2.0, 7.0, 5.0, 6.0}));
            CHECK((tf.rank(name, RankMethod::Dense) == std::vector<double>{2.0, 1.0, 3.0, 1.0, 4.0, 3.0, 3.0}));
        }
        const std::vector<double> g = tf.rank("gaps", RankMethod::Max);             // NaN and null take no rank; -0.0 ties 0.0
        CHECK(g.size() == 7 && std::isnan(g[1]) && std::isnan(g[3]) && g[0] == 5.0 && g[2] == 4.0 && g[4] == 4.0 && g[5] == 2.0 && g[6] == 2.0);
    }
    const std::vector<double> x = {3.0, 1.0, 4.0, 1.0, 5.0};
    const pandrs_hip_column col{x.data(), nullptr, PANDRS_HIP_F64, 0};
    double out[5] = {0, 0, 0, 0, 0};
    CHECK(pandrs_hip_rank(detail::context(), PANDRS_HIP_MEM_HOST, &col, 5, 5, PANDRS_HIP_MEM_HOST, out) == PANDRS_HIP_ERR_INVALID_ARGUMENT);
    CHECK(pandrs_hip_rank(detail::context(), PANDRS_HIP_MEM_HOST, &col, 5, PANDRS_HIP_RANK_DENSE, PANDRS_HIP_MEM_HOST, out) == PANDRS_HIP_OK);
    CHECK(out[0] == 2.0 && out[1] == 1.0 && out[2] == 3.0 && out[3] == 1.0 && out[4] == 4.0);
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
