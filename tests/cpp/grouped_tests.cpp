// GroupBy::cumsum / cummax / cummin / cumcount / row_number / shift / diff / pct_change through the C++ host mirror
// (include/pandrs_hip.hpp) over libpandrs_hip.so: for every group the frame-level method over the group's rows in ascending
// row order (pandrs_hip_grouped, pandrs_hip.h), host and resident, Int64 values, string keys, null masks, two keys.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "pandrs_hip.hpp"

using namespace pandrs;

static int g_failed = 0, g_run = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("    CHECK failed: %s  (%s:%d)\n", #cond, __FILE__, __LINE__); g_failed++; } } while (0)
#define RUN(fn) do { g_run++; std::printf("test %s\n", #fn); try { fn(); } catch (const std::exception &e) { std::printf("    threw: %s\n", e.what()); g_failed++; } } while (0)

// rows 0 .. 7, keys a b a b a c b a: group a = rows 0 2 4 7, b = rows 1 3 6, c = row 5
static OptimizedDataFrame test_df(bool resident) {
    OptimizedDataFrame df;
    df.add_column("k", StringColumn(std::vector<std::string>{"a", "b", "a", "b", "a", "c", "b", "a"}));
    df.add_column("id", Int64Column(std::vector<int64_t>{1, 2, 1, 2, 1, 3, 2, 1}));
    df.add_column("x", Float64Column(std::vector<double>{1.0, 10.0, 2.0, 20.0, 3.0, 100.0, 30.0, 4.0}));
    df.add_column("i", Int64Column::with_nulls({7, 1, 100, -3, 2, 9, 5, 1}, {false, false, true, false, false, false, false, false}));
    df.add_column("flag", BooleanColumn(std::vector<bool>(8, true)));
    if (resident) df.make_resident();
    return df;
}

static void test_errors_before_any_device_call() {
    auto df = test_df(false);
    auto g = df.group_by({"k"});
    try { g.cumsum("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { g.shift("nope", 1); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { g.cummax("flag"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type && std::string(e.what()) == "Column 'flag' is not a numeric type"); }
    try { g.cumcount("k"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { g.diff("k", 1); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { g.pct_change("flag", 1); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    OptimizedDataFrame empty;
    empty.add_column("k", Int64Column(std::vector<int64_t>{}));
    empty.add_column("v", Float64Column(std::vector<double>{}));
    auto ge = empty.group_by({"k"});
    CHECK(ge.cumsum("v").empty() && ge.cummin("v").empty() && ge.cumcount("v").empty() && ge.row_number().empty() && ge.shift("v", 1).empty() &&
          ge.diff("v", 1).empty() && ge.pct_change("v", 2).empty());
    CHECK(PANDRS_HIP_GROUPED_CUM_SUM == 0 && PANDRS_HIP_GROUPED_CUM_MAX == 1 && PANDRS_HIP_GROUPED_CUM_MIN == 2 && PANDRS_HIP_GROUPED_CUM_COUNT == 3 &&
          PANDRS_HIP_GROUPED_ROW_NUMBER == 4 && PANDRS_HIP_GROUPED_SHIFT == 5 && PANDRS_HIP_GROUPED_DIFF == 6 && PANDRS_HIP_GROUPED_PCT_CHANGE == 7);
    double out[1] = {0};
    CHECK(pandrs_hip_grouped(nullptr, PANDRS_HIP_MEM_HOST, nullptr, 1, PANDRS_HIP_GROUPED_ROW_NUMBER, 0, PANDRS_HIP_MEM_HOST, out, nullptr, nullptr) ==
          PANDRS_HIP_ERR_NOT_INITIALIZED);
}

static void test_answers_per_group() {
    for (int res = 0; res < 2; res++) {
        auto df = test_df(res);
        for (const char *key : {"k", "id"}) {
            auto g = df.group_by({key});
            CHECK(g.cumsum("x") == (std::vector<double>{1.0, 10.0, 3.0, 30.0, 6.0, 100.0, 60.0, 10.0}));
            CHECK(g.cummax("x") == (std::vector<double>{1.0, 10.0, 2.0, 20.0, 3.0, 100.0, 30.0, 4.0}));
            CHECK(g.cummin("x") == (std::vector<double>{1.0, 10.0, 1.0, 10.0, 1.0, 100.0, 10.0, 1.0}));
            CHECK(g.cumcount("x") == (std::vector<size_t>{1, 1, 2, 2, 3, 1, 3, 4}));
            CHECK(g.row_number() == (std::vector<size_t>{0, 0, 1, 1, 2, 0, 2, 3}));
            auto s = g.shift("x", 1);
            CHECK(s.size() == 8 && !s[0] && !s[1] && s[2] == 1.0 && s[3] == 10.0 && s[4] == 2.0 && !s[5] && s[6] == 20.0 && s[7] == 3.0);
            auto back = g.shift("x", -2);
            CHECK(back[0] == 3.0 && back[1] == 30.0 && back[2] == 4.0 && !back[3] && !back[4] && !back[5] && !back[6] && !back[7]);
            auto d = g.diff("x", 1);
            CHECK(std::isnan(d[0]) && std::isnan(d[1]) && d[2] == 1.0 && d[3] == 10.0 && d[4] == 1.0 && std::isnan(d[5]) && d[6] == 10.0 && d[7] == 1.0);
            auto far = g.diff("x", 99);
            CHECK(far.size() == 8 && std::isnan(far[0]) && std::isnan(far[7]));
            auto p = g.pct_change("x", 2);
            CHECK(std::isnan(p[0]) && std::isnan(p[2]) && p[4] == (3.0 - 1.0) / 1.0 && p[6] == (30.0 - 10.0) / 10.0 && p[7] == (4.0 - 2.0) / 2.0 && std::isnan(p[5]));
        }
    }
}

static void test_null_masks_int64_and_two_keys() {
    for (int res = 0; res < 2; res++) {
        auto df = test_df(res);
        auto g = df.group_by({"k"});
        auto cs = g.cumsum("i");                              // group a = 7, null, 2, 1: the null row is skipped and answers NaN
        CHECK(cs[0] == 7.0 && std::isnan(cs[2]) && cs[4] == 9.0 && cs[7] == 10.0 && cs[1] == 1.0 && cs[3] == -2.0 && cs[6] == 3.0 && cs[5] == 9.0);
        CHECK(g.cumcount("i") == (std::vector<size_t>{1, 1, 1, 2, 2, 1, 3, 3}));
        auto sh = g.shift("i", 1);
        CHECK(!sh[0] && sh[2] == 7.0 && !sh[4] && sh[7] == 2.0 && sh[3] == 1.0);       // row 4's source is the null row 2
        auto di = g.diff("i", 1);
        CHECK(std::isnan(di[0]) && std::isnan(di[2]) && std::isnan(di[4]) && di[7] == -1.0 && di[3] == -4.0);
        auto g2 = df.group_by({"k", "id"});                   // the same groups through a two-key grouping
        CHECK(g2.cumsum("x") == g.cumsum("x") && g2.row_number() == g.row_number());
    }
    auto z = OptimizedDataFrame();
    z.add_column("k", Int64Column(std::vector<int64_t>{1, 2, 1, 2}));
    z.add_column("x", Float64Column(std::vector<double>{-0.0, NAN, -0.0, 5.0}));
    auto gz = z.group_by({"k"});
    auto s = gz.cumsum("x");                                   // a group of only -0.0 gives +0.0; a NaN poisons its own group only
    CHECK(s[0] == 0.0 && !std::signbit(s[0]) && !std::signbit(s[2]) && std::isnan(s[1]) && std::isnan(s[3]));
    auto m = gz.cummax("x");                                   // a leading NaN: the fold's -inf shows
    CHECK(std::isinf(m[1]) && m[1] < 0 && m[3] == 5.0);
}

int main() {
    RUN(test_errors_before_any_device_call);
    int32_t n_dev = 0;
    if (pandrs_hip_init(nullptr) != PANDRS_HIP_OK || pandrs_hip_device_count(&n_dev) != PANDRS_HIP_OK || n_dev == 0) {
        std::printf("%d tests, %d failed checks\n", g_run, g_failed);
        std::fprintf(stderr, "no HIP device available: %s\n", pandrs_hip_last_error());
        return g_failed ? 2 : 1;
    }
    RUN(test_answers_per_group);
    RUN(test_null_masks_int64_and_two_keys);
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
