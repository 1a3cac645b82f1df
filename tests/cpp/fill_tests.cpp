// PandasCompatExt::fillna / fillna_method / interpolate / ffill / bfill (src/dataframe/pandas_compat/functions.rs:789-918,
// :3626-3683) through the C++ host mirror (include/pandrs_hip.hpp) over libpandrs_hip.so: the reference's known answers
// (functions.rs:4751-4970, :8007-8050, :8489), host and resident, and the Int64 / null-mask extensions of pandrs_hip.h.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "pandrs_hip.hpp"

using namespace pandrs;

static int g_failed = 0, g_run = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("    CHECK failed: %s  (%s:%d)\n", #cond, __FILE__, __LINE__); g_failed++; } } while (0)
#define RUN(fn) do { g_run++; std::printf("test %s\n", #fn); try { fn(); } catch (const std::exception &e) { std::printf("    threw: %s\n", e.what()); g_failed++; } } while (0)

static OptimizedDataFrame frame_of(const std::vector<double> &a, bool resident) {
    OptimizedDataFrame df;
    df.add_column("id", Int64Column(std::vector<int64_t>(a.size(), 7)));
    df.add_column("a", Float64Column(a));
    df.add_column("s", StringColumn(std::vector<std::string>(a.size(), "x")));
    df.add_column("b", BooleanColumn(std::vector<bool>(a.size(), true)));
    if (resident) df.make_resident();
    return df;
}

// the "a" column of a result: position 1, Float64; NaN in `want` = the row is still missing (NaN cell, bit set)
static bool column_is(const OptimizedDataFrame &r, const std::vector<double> &want) {
    if (r.column_names != std::vector<std::string>{"id", "a", "s", "b"} || r.column("a").index() != 1) return false;
    const Float64Column &c = std::get<Float64Column>(r.column("a"));
    if (c.data.size() != want.size()) return false;
    bool any = false;
    for (size_t i = 0; i < want.size(); i++) {
        const bool gone = std::isnan(want[i]);
        any |= gone;
        if (gone ? !(std::isnan(c.data[i]) && detail::bit_at(c.null_mask, i)) : !(c.data[i] == want[i] && !detail::bit_at(c.null_mask, i))) return false;
    }
    return any || c.null_mask.empty();
}

static void test_errors_before_any_device_call() {
    auto df = frame_of({1.0, NAN, 3.0}, false);
    try { df.ffill("nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.fillna_method("nope", "invalid"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.bfill("s"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.interpolate("b"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type && std::string(e.what()) == "Column 'b' is not a numeric type"); }
    try { df.fillna("s", 0.0); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    try { df.fillna_method("a", "invalid"); CHECK(false); }                             // functions.rs:4877-4887
    catch (const Error &e) { CHECK(e.kind == Error::InvalidValue && std::string(e.what()) == "Invalid fill method: 'invalid'. Use 'ffill' or 'bfill'."); }
    try { df.fillna("id", 0.5); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::InvalidValue); }
    OptimizedDataFrame empty;
    empty.add_column("v", Float64Column(std::vector<double>{}));
    CHECK(empty.ffill("v").row_count() == 0 && empty.interpolate("v").column_names == std::vector<std::string>{"v"});
    CHECK(PANDRS_HIP_FILL_FFILL == 0 && PANDRS_HIP_FILL_BFILL == 1 && PANDRS_HIP_FILL_LINEAR == 2 && PANDRS_HIP_FILL_VALUE == 3);
}

static void test_known_answers() {
    for (int res = 0; res < 2; res++) {
        CHECK(column_is(frame_of({1.0, NAN, 3.0, NAN, 5.0}, res).fillna("a", 0.0), {1.0, 0.0, 3.0, 0.0, 5.0}));                  // :4751
        CHECK(column_is(frame_of({1.0, NAN, 3.0}, res).fillna("a", -999.0), {1.0, -999.0, 3.0}));                                // :4767
        CHECK(column_is(frame_of({1.0, NAN, NAN, 4.0, NAN, 6.0}, res).fillna_method("a", "ffill"), {1.0, 1.0, 1.0, 4.0, 4.0, 6.0}));   // :4780
        CHECK(column_is(frame_of({1.0, NAN, NAN, 4.0, NAN, 6.0}, res).fillna_method("a", "bfill"), {1.0, 4.0, 4.0, 4.0, 6.0, 6.0}));   // :4805
        CHECK(column_is(frame_of({1.0, NAN, NAN, 4.0, NAN, 6.0}, res).fillna_method("a", "forward"), {1.0, 1.0, 1.0, 4.0, 4.0, 6.0}));
        CHECK(column_is(frame_of({1.0, NAN, NAN, 4.0, NAN, 6.0}, res).fillna_method("a", "backward"), {1.0, 4.0, 4.0, 4.0, 6.0, 6.0}));
        CHECK(column_is(frame_of({NAN, NAN, 3.0, NAN, 5.0}, res).fillna_method("a", "ffill"), {NAN, NAN, 3.0, 3.0, 5.0}));       // :4829
        CHECK(column_is(frame_of({1.0, NAN, 3.0, NAN, NAN}, res).fillna_method("a", "bfill"), {1.0, 3.0, 3.0, NAN, NAN}));       // :4853
        CHECK(column_is(frame_of({1.0, NAN, NAN, 4.0, NAN, 6.0}, res).interpolate("a"), {1.0, 2.0, 3.0, 4.0, 5.0, 6.0}));        // :4890
        CHECK(column_is(frame_of({2.0, NAN, 8.0}, res).interpolate("a"), {2.0, 5.0, 8.0}));                                      // :4914
        CHECK(column_is(frame_of({NAN, 2.0, NAN, 4.0, NAN}, res).interpolate("a"), {NAN, 2.0, 3.0, 4.0, NAN}));                  // :4931
        CHECK(column_is(frame_of({1.0, 2.0, 3.0, 4.0}, res).interpolate("a"), {1.0, 2.0, 3.0, 4.0}));                            // :4956
        CHECK(column_is(frame_of({1.0, NAN, NAN, 4.0, NAN}, res).ffill("a"), {1.0, 1.0, 1.0, 4.0, 4.0}));                        // :8007
        CHECK(column_is(frame_of({NAN, NAN, 3.0, NAN, 5.0}, res).bfill("a"), {3.0, 3.0, 3.0, 5.0, 5.0}));                        // :8030
        CHECK(column_is(frame_of({1.0, NAN, 3.0, NAN}, res).fillna("a", 0.0), {1.0, 0.0, 3.0, 0.0}));                            // :8489
    }
}

static void test_int64_and_null_masks() {
    for (int res = 0; res < 2; res++) {
        OptimizedDataFrame df;
        df.add_column("i", Int64Column::with_nulls({7, 0, 0, -3, 0}, {false, true, true, false, true}));
        df.add_column("f", Float64Column::with_nulls({1.0, 99.0, NAN, 3.0, 4.0}, {false, true, false, false, false}));
        if (res) df.make_resident();
        auto f = df.ffill("i");
        CHECK(f.column("i").index() == 0 && std::get<Int64Column>(f.column("i")).data == (std::vector<int64_t>{7, 7, 7, -3, -3}) &&
              std::get<Int64Column>(f.column("i")).null_mask.empty());
        auto b = df.bfill("i");
        const Int64Column &bi = std::get<Int64Column>(b.column("i"));
        CHECK(bi.data == (std::vector<int64_t>{7, -3, -3, -3, 0}) && bi.null_mask == std::vector<uint8_t>{0x10});
        auto v = df.fillna("i", -5.0);
        CHECK(std::get<Int64Column>(v.column("i")).data == (std::vector<int64_t>{7, -5, -5, -3, -5}));
        auto l = df.interpolate("i");
        CHECK(l.column("i").index() == 1 && l.column_names == (std::vector<std::string>{"i", "f"}));
        const Float64Column &li = std::get<Float64Column>(l.column("i"));
        CHECK(li.data[0] == 7.0 && li.data[1] == 7.0 + (-10.0 * 1.0) / 3.0 && li.data[2] == 7.0 + (-10.0 * 2.0) / 3.0 && li.data[3] == -3.0 &&
              std::isnan(li.data[4]) && li.null_mask == std::vector<uint8_t>{0x10});
        auto g = df.ffill("f");                                 // the null over 99.0 is never a source
        CHECK(std::get<Float64Column>(g.column("f")).data == (std::vector<double>{1.0, 1.0, 1.0, 3.0, 4.0}) &&
              std::get<Float64Column>(g.column("f")).null_mask.empty());
    }
    const std::vector<double> x = {1.0, NAN, 3.0};
    const pandrs_hip_column col{x.data(), nullptr, PANDRS_HIP_F64, 0};
    double out[3] = {0, 0, 0};
    int64_t missing = -1;
    CHECK(pandrs_hip_fill(detail::context(), PANDRS_HIP_MEM_HOST, &col, 3, 4, 0, PANDRS_HIP_MEM_HOST, out, nullptr, &missing) == PANDRS_HIP_ERR_INVALID_ARGUMENT);
    CHECK(pandrs_hip_fill(detail::context(), PANDRS_HIP_MEM_HOST, &col, 3, PANDRS_HIP_FILL_LINEAR, 0, PANDRS_HIP_MEM_HOST, out, nullptr, &missing) == PANDRS_HIP_OK);
    CHECK(out[0] == 1.0 && out[1] == 2.0 && out[2] == 3.0 && missing == 0);
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
    RUN(test_int64_and_null_masks);
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
