// OptimizedDataFrame::sort_by / sort_by_columns (src/optimized/split_dataframe/sort.rs:18-272) through the C++ host
// mirror (include/pandrs_hip.hpp) over libpandrs_hip.so.  The expected order is sort.rs's comparator restated
// here with std::stable_sort (slice::sort_by is stable), plus the header's NaN rule.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <optional>
#include <string>
#include <vector>

#include "pandrs_hip.hpp"

using namespace pandrs;

static int g_failed = 0, g_run = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("    CHECK failed: %s  (%s:%d)\n", #cond, __FILE__, __LINE__); g_failed++; } } while (0)
#define RUN(fn) do { g_run++; std::printf("test %s\n", #fn); try { fn(); } catch (const std::exception &e) { std::printf("    threw: %s\n", e.what()); g_failed++; } } while (0)

// (None, _) => Greater before the direction; NaN after every number, before nulls; -0.0 == 0.0
static int cmp_f64(std::optional<double> a, std::optional<double> b, bool asc) {
    if (!a && !b) return 0;
    if (!a) return 1;
    if (!b) return -1;
    const bool na = std::isnan(*a), nb = std::isnan(*b);
    if (na || nb) return na && nb ? 0 : (na ? 1 : -1);
    const int c = *a < *b ? -1 : (*a > *b ? 1 : 0);
    return asc ? c : -c;
}
static int cmp_str(std::optional<std::string> a, std::optional<std::string> b, bool asc) {
    if (!a && !b) return 0;
    if (!a) return 1;
    if (!b) return -1;
    const int c = a->compare(*b) < 0 ? -1 : (a->compare(*b) > 0 ? 1 : 0);
    return asc ? c : -c;
}

static OptimizedDataFrame sample_frame() {
    OptimizedDataFrame df;
    df.add_column("id", Int64Column({0, 1, 2, 3, 4, 5, 6, 7, 8, 9}));
    df.add_column("x", Float64Column::with_nulls({2.0, NAN, -0.0, 1.5, 0.0, 2.0, 0.0, -3.0, NAN, 1.5},
                                                 {false, false, false, false, true, false, false, false, false, true}));
    df.add_column("s", StringColumn::with_nulls({"b", "\xc3\xa9", "a", "", "b", "Z", "a", "ab", "b", "a"},
                                                {false, false, false, false, false, false, true, false, false, false}));
    df.add_column("flag", BooleanColumn({true, false, true, false, true, false, true, false, true, false}));
    return df;
}

static void test_errors_before_any_device_call() {
    auto df = sample_frame();
    try { df.sort_by_columns({}); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::EmptyColumnList); }
    try { df.sort_by("nope", true); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.sort_by_columns({"x", "s"}, {true}); CHECK(false); }
    catch (const Error &e) {
        CHECK(e.kind == Error::InconsistentArrayLengths);
        CHECK(std::string(e.what()).find("expected 2, found 1") != std::string::npos);
    }
}

static void test_sort_by_columns_matches_the_comparator() {
    auto df = sample_frame();
    auto &x = std::get<Float64Column>(df.column("x"));
    auto &s = std::get<StringColumn>(df.column("s"));
    std::vector<int64_t> want(df.row_count());
    for (size_t i = 0; i < want.size(); i++) want[i] = (int64_t)i;
    auto xv = [&](int64_t i) { return detail::bit_at(x.null_mask, i) ? std::optional<double>() : std::optional<double>(x.data[i]); };
    auto sv = [&](int64_t i) { return detail::bit_at(s.null_mask, i) ? std::optional<std::string>() : std::optional<std::string>(s.get(i)); };
    std::stable_sort(want.begin(), want.end(), [&](int64_t a, int64_t b) {
        int c = cmp_str(sv(a), sv(b), false);
        if (c == 0) c = cmp_f64(xv(a), xv(b), true);
        return c < 0;
    });
    auto r = df.sort_by_columns({"s", "x"}, {false, true});
    CHECK(r.column_count() == 4 && r.column_names == df.column_names);
    auto &id = std::get<Int64Column>(r.column("id"));
    CHECK(id.data == want);
    auto &rx = std::get<Float64Column>(r.column("x"));
    CHECK(rx.null_mask.empty());
    for (size_t i = 0; i < want.size(); i++) {
        auto v = xv(want[i]);
        CHECK(v ? (std::isnan(*v) ? std::isnan(rx.data[i]) : rx.data[i] == *v) : rx.data[i] == 0.0);   // a null becomes 0.0
        auto sw = sv(want[i]);
        CHECK(std::get<StringColumn>(r.column("s")).get(i) == (sw ? *sw : std::string()));   // ... and ""
    }
    // one key, descending: ties keep row order
    auto r2 = df.sort_by("flag", false);
    CHECK(std::get<Int64Column>(r2.column("id")).data == (std::vector<int64_t>{0, 2, 4, 6, 8, 1, 3, 5, 7, 9}));
    // the resident frame gives the same answer
    auto dr = sample_frame();
    dr.make_resident();
    CHECK(std::get<Int64Column>(dr.sort_by_columns({"s", "x"}, {false, true}).column("id")).data == want);
    // no rows: a frame without columns
    OptimizedDataFrame empty;
    empty.add_column("a", Int64Column(std::vector<int64_t>{}));
    CHECK(empty.sort_by("a", true).column_count() == 0);
}

int main() {
    RUN(test_errors_before_any_device_call);
    int32_t n_dev = 0;
    if (pandrs_hip_init(nullptr) != PANDRS_HIP_OK || pandrs_hip_device_count(&n_dev) != PANDRS_HIP_OK || n_dev == 0) {
        std::printf("%d tests, %d failed checks\n", g_run, g_failed);
        std::fprintf(stderr, "no HIP device available: %s\n", pandrs_hip_last_error());
        return g_failed ? 2 : 1;
    }
    RUN(test_sort_by_columns_matches_the_comparator);
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
