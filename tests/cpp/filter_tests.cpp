// OptimizedDataFrame::filter / filter_rows / par_filter / select_by_mask / select (src/optimized/split_dataframe/
// data_ops.rs:15-121, row_ops.rs:26-130, parallel.rs:21-230, select.rs:150-167) through the C++ host mirror
// (include/pandrs_hip.hpp) over libpandrs_hip.so.  The expected rows are the reference's loop restated here:
// row i is kept iff the condition is Some(true); nulls become 0 / 0.0 / "" / false.
#include <cstdio>
#include <string>
#include <vector>

#include "pandrs_hip.hpp"

using namespace pandrs;

static int g_failed = 0, g_run = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("    CHECK failed: %s  (%s:%d)\n", #cond, __FILE__, __LINE__); g_failed++; } } while (0)
#define RUN(fn) do { g_run++; std::printf("test %s\n", #fn); try { fn(); } catch (const std::exception &e) { std::printf("    threw: %s\n", e.what()); g_failed++; } } while (0)

static BooleanColumn bool_with_nulls(const std::vector<bool> &values, const std::vector<bool> &nulls) {
    BooleanColumn c(values);
    c.null_mask = detail::create_bitmask(nulls);
    return c;
}

static OptimizedDataFrame sample_frame() {
    OptimizedDataFrame df;
    df.add_column("id", Int64Column::with_nulls({0, 1, 2, 3, 4, 5, 6, 7, 8, 9},
                                                {false, false, false, true, false, false, false, false, false, false}));
    df.add_column("x", Float64Column::with_nulls({2.0, 0.5, -0.0, 1.5, 0.0, 2.0, 0.25, -3.0, 9.0, 1.5},
                                                 {false, false, false, false, true, false, false, false, false, true}));
    df.add_column("s", StringColumn::with_nulls({"b", "\xc3\xa9", "a", "", "b", "Z", "a", "ab", "b", "a"},
                                                {false, false, true, false, false, false, false, false, false, false}));
    df.add_column("flag", bool_with_nulls({true, false, true, true, true, false, true, false, true, true},
                                                    {false, false, false, false, false, false, true, false, false, false}));
    df.add_column("b", BooleanColumn({true, true, false, true, false, false, true, true, true, false}));
    return df;
}

static void test_errors_before_any_device_call() {
    auto df = sample_frame();
    try { df.filter("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.par_filter("id"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnTypeMismatch); }
    try { df.filter_rows("s"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnTypeMismatch); }
    try { df.select_by_mask({true, false}); CHECK(false); }
    catch (const Error &e) {
        CHECK(e.kind == Error::Format);
        CHECK(std::string(e.what()) == "Mask length (2) does not match DataFrame row count (10)");
    }
    try { df.select({"id", "nonexistent"}); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    auto sel = df.select({"x", "id"});
    CHECK(sel.column_names == (std::vector<std::string>{"x", "id"}));
    CHECK(!std::get<Float64Column>(sel.column("x")).null_mask.empty());     // select keeps null masks
    OptimizedDataFrame empty;
    empty.add_column("a", Int64Column(std::vector<int64_t>{}));
    empty.add_column("f", BooleanColumn(std::vector<bool>{}));
    CHECK(empty.filter("f").column_count() == 2 && empty.par_filter("f").row_count() == 0);
    CHECK(empty.select_by_mask({}).column_count() == 0);
}

static void test_filter_matches_the_reference_loop() {
    // flag: Some(true) at rows 0, 2, 3, 4, 8, 9 (row 6 is null, so dropped)
    const std::vector<int64_t> rows = {0, 2, 3, 4, 8, 9};
    for (int resident = 0; resident < 2; resident++) {
        auto df = sample_frame();
        if (resident) df.make_resident();
        for (int m = 0; m < 3; m++) {
            auto r = m == 0 ? df.filter("flag") : (m == 1 ? df.filter_rows("flag") : df.par_filter("flag"));
            CHECK(r.column_names == df.column_names && r.row_count() == rows.size());
            CHECK(std::get<Int64Column>(r.column("id")).data == (std::vector<int64_t>{0, 2, 0, 4, 8, 9}));      // null id 3 -> 0
            auto &x = std::get<Float64Column>(r.column("x"));
            CHECK(x.data == (std::vector<double>{2.0, -0.0, 1.5, 0.0, 9.0, 0.0}) && x.null_mask.empty());
            auto &s = std::get<StringColumn>(r.column("s"));
            CHECK(s.get(0) == "b" && s.get(1) == "" && s.get(2) == "" && s.get(5) == "a");
            auto &b = std::get<BooleanColumn>(r.column("b"));
            CHECK(b.get(0) && !b.get(1) && b.get(2) && !b.get(3) && b.get(4) && !b.get(5));
            auto &f = std::get<BooleanColumn>(r.column("flag"));
            for (size_t k = 0; k < rows.size(); k++) CHECK(f.get(k));
        }
        // select_by_mask: a host mask, the frame's own columns (resident or not)
        auto r = df.select_by_mask({false, true, false, false, false, false, false, true, false, true});
        CHECK(std::get<Int64Column>(r.column("id")).data == (std::vector<int64_t>{1, 7, 9}));
        CHECK(std::get<Float64Column>(r.column("x")).data == (std::vector<double>{0.5, -3.0, 0.0}));
        // nothing selected: filter / par_filter keep every column with 0 rows, select_by_mask has no columns
        OptimizedDataFrame none;
        none.add_column("v", Float64Column({1.0, 2.0, 3.0}));
        none.add_column("c", bool_with_nulls({false, true, false}, {false, true, false}));
        if (resident) none.make_resident();
        CHECK(none.filter("c").column_count() == 2 && none.filter("c").row_count() == 0);
        CHECK(none.par_filter("c").column_count() == 2 && none.par_filter("c").row_count() == 0);
        CHECK(none.select_by_mask({false, false, false}).column_count() == 0);
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
    RUN(test_filter_matches_the_reference_loop);
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
