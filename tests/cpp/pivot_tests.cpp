// PandasCompatExt::crosstab / unstack / pivot (src/dataframe/pandas_compat/functions.rs:2138-2183, :2471-2527) and
// DataFrame::pivot_table (src/pivot/mod.rs:12-250) through the C++ host mirror (include/pandrs_hip.hpp) over libpandrs_hip.so: the
// reference's tests test_crosstab (:6650), test_unstack (:7052), test_pivot (:7097) and the frame of examples/pivot_example.rs,
// with the full tables the reference's loops give for those inputs.
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
using Numbers = std::vector<double>;

static Strings strings_of(const OptimizedDataFrame &df, const std::string &name) {
    const auto &c = std::get<StringColumn>(df.column(name));
    Strings out;
    for (size_t i = 0; i < c.len(); i++) out.push_back(c.get(i));
    return out;
}
static const Float64Column &numbers_of(const OptimizedDataFrame &df, const std::string &name) { return std::get<Float64Column>(df.column(name)); }
static bool null_at(const Float64Column &c, size_t i) { return !c.null_mask.empty() && ((c.null_mask[i >> 3] >> (i & 7)) & 1); }

static OptimizedDataFrame sales() {
    OptimizedDataFrame df;
    df.add_column("category", StringColumn({"A", "B", "A", "C", "B", "A", "C"}));
    df.add_column("region", StringColumn({"East", "West", "West", "East", "East", "East", "North"}));
    df.add_column("sales", Float64Column({100.0, 200.0, 150.0, 300.0, 250.0, 50.0, 75.0}));
    df.add_column("units", Int64Column::with_nulls({1, 2, 3, 4, 5, 6, 7}, {false, false, false, false, true, false, false}));
    df.add_column("flag", BooleanColumn({true, false, true, false, true, false, true}));
    return df;
}

static void test_errors_before_any_device_call() {
    auto df = sales();
    try { df.crosstab("nope", "region"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.crosstab("category", "nope"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.pivot_table("category", "region", "nope", AggFunction::Sum); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.unstack("nope", "region", "sales"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.pivot("category", "nope", "sales"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::ColumnNotFound); }
    try { df.pivot_table("category", "region", "region", AggFunction::Sum); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type && std::string(e.what()) == "Column 'region' is not a numeric type"); }
    try { df.unstack("category", "region", "flag"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::Type); }
    // no rows: only the (empty) index column, no device call
    OptimizedDataFrame empty;
    empty.add_column("a", StringColumn(Strings{}));
    empty.add_column("b", StringColumn(Strings{}));
    empty.add_column("v", Float64Column(Numbers{}));
    CHECK(empty.crosstab("a", "b").column_count() == 1 && empty.crosstab("a", "b").row_count() == 0);
    CHECK(empty.pivot_table("a", "b", "v", AggFunction::Mean).column_count() == 1 && empty.unstack("a", "b", "v").column_names == Strings{"a"});
    // AggFunction: the names and from_str of pivot/mod.rs:25-48
    AggFunction f = AggFunction::Sum;
    CHECK(agg_function_from_str("AVG", &f) && f == AggFunction::Mean && agg_function_from_str("average", &f) && f == AggFunction::Mean);
    CHECK(agg_function_from_str("Minimum", &f) && f == AggFunction::Min && agg_function_from_str("maximum", &f) && f == AggFunction::Max);
    CHECK(agg_function_from_str("count", &f) && f == AggFunction::Count && agg_function_from_str("sum", &f) && f == AggFunction::Sum);
    CHECK(!agg_function_from_str("median", &f) && std::string(agg_function_name(AggFunction::Mean)) == "mean" && std::string(agg_function_name(AggFunction::Count)) == "count");
    CHECK(PANDRS_HIP_PIVOT_ROWS == 0 && PANDRS_HIP_PIVOT_COUNT == 5 && PANDRS_HIP_PIVOT_LAST == 6);
}

static void test_crosstab() {                            // :6650-6689
    OptimizedDataFrame df;
    df.add_column("gender", StringColumn({"M", "F", "M", "F", "M"}));
    df.add_column("category", StringColumn({"A", "A", "B", "B", "A"}));
    const auto r = df.crosstab("gender", "category");
    CHECK(r.contains_column("gender") && r.contains_column("A") && r.contains_column("B"));
    CHECK((r.column_names == Strings{"gender", "A", "B"}) && (strings_of(r, "gender") == Strings{"F", "M"}));
    CHECK((numbers_of(r, "A").data == Numbers{1.0, 2.0}) && (numbers_of(r, "B").data == Numbers{1.0, 1.0}));
}

static void test_unstack() {                             // :7052-7095
    OptimizedDataFrame df;
    df.add_column("idx", StringColumn({"A", "A", "B", "B"}));
    df.add_column("col", StringColumn({"X", "Y", "X", "Y"}));
    df.add_column("val", Float64Column({1.0, 2.0, 3.0, 4.0}));
    const auto r = df.unstack("idx", "col", "val");
    CHECK(r.contains_column("idx") && r.contains_column("X") && r.contains_column("Y") && r.row_count() == 2);
    CHECK((numbers_of(r, "X").data == Numbers{1.0, 3.0}) && (numbers_of(r, "Y").data == Numbers{2.0, 4.0}));
}

static void test_pivot() {                               // :7097-7139
    OptimizedDataFrame df;
    df.add_column("date", StringColumn({"Mon", "Mon", "Tue", "Tue"}));
    df.add_column("type", StringColumn({"A", "B", "A", "B"}));
    df.add_column("value", Float64Column({10.0, 20.0, 30.0, 40.0}));
    const auto r = df.pivot("date", "type", "value");
    CHECK(r.contains_column("date") && r.contains_column("A") && r.contains_column("B"));
    CHECK((numbers_of(r, "A").data == Numbers{10.0, 30.0}) && (numbers_of(r, "B").data == Numbers{20.0, 40.0}));
}

static void test_pivot_table() {                         // pivot/mod.rs:107-228 on the frame of examples/pivot_example.rs
    const auto df = sales();
    const auto s = df.pivot_table("category", "region", "sales", AggFunction::Sum);
    CHECK((s.column_names == Strings{"category", "East", "North", "West"}) && (strings_of(s, "category") == Strings{"A", "B", "C"}));
    const auto &east = numbers_of(s, "East"), &north = numbers_of(s, "North"), &west = numbers_of(s, "West");
    CHECK((east.data == Numbers{150.0, 250.0, 300.0}) && east.null_mask.empty());
    CHECK(null_at(north, 0) && null_at(north, 1) && !null_at(north, 2) && north.data[2] == 75.0 && std::isnan(north.data[0]));
    CHECK(west.data[0] == 150.0 && west.data[1] == 200.0 && null_at(west, 2));
    const auto m = df.pivot_table("category", "region", "sales", AggFunction::Mean);
    CHECK(numbers_of(m, "East").data == (Numbers{75.0, 250.0, 300.0}));
    CHECK(numbers_of(df.pivot_table("category", "region", "sales", AggFunction::Min), "East").data == (Numbers{50.0, 250.0, 300.0}));
    CHECK(numbers_of(df.pivot_table("category", "region", "sales", AggFunction::Max), "East").data == (Numbers{100.0, 250.0, 300.0}));
    CHECK(numbers_of(df.pivot_table("category", "region", "sales", AggFunction::Count), "East").data == (Numbers{2.0, 1.0, 1.0}));
    // Int64 values with a null cell: skipped by Sum, counted by Count; a cell of nulls only: Sum 0.0, Mean 0.0
    CHECK(numbers_of(df.pivot_table("category", "region", "units", AggFunction::Sum), "East").data == (Numbers{7.0, 0.0, 4.0}));
    CHECK(numbers_of(df.pivot_table("category", "region", "units", AggFunction::Mean), "East").data == (Numbers{3.5, 0.0, 4.0}));
    CHECK(numbers_of(df.pivot_table("category", "region", "units", AggFunction::Count), "East").data == (Numbers{2.0, 1.0, 1.0}));
}

static void test_other_key_types_and_missing_cells() {
    OptimizedDataFrame df;
    df.add_column("i", Int64Column::with_nulls({10, 9, 10, -2, 9, 10}, {false, false, false, false, true, false}));
    df.add_column("x", Float64Column({1.5, NAN, 1.5, 2.0, 2.0, NAN}));
    df.add_column("flag", BooleanColumn({true, false, true, false, true, false}));
    df.add_column("s", StringColumn::with_nulls({"b", "", "b", "a", "a", "a"}, {false, false, false, false, false, true}));
    df.add_column("v", Float64Column({1.0, 2.0, 3.0, 4.0, 5.0, 6.0}));
    // numeric labels are stringified and ordered as strings: "-2" < "10" < "9" < "NaN"
    const auto c = df.crosstab("i", "x");
    CHECK((strings_of(c, "i") == Strings{"-2", "10", "9", "NaN"}) && (c.column_names == Strings{"i", "1.5", "2", "NaN"}));
    CHECK((numbers_of(c, "1.5").data == Numbers{0.0, 2.0, 0.0, 0.0}) && (numbers_of(c, "2").data == Numbers{1.0, 0.0, 0.0, 1.0}));
    CHECK((numbers_of(c, "NaN").data == Numbers{0.0, 1.0, 1.0, 0.0}));
    const auto b = df.crosstab("flag", "s");                // the null cell of s reads "", like its literal "": the counts add
    CHECK((strings_of(b, "flag") == Strings{"false", "true"}) && (b.column_names == Strings{"flag", "", "a", "b"}));
    CHECK((numbers_of(b, "").data == Numbers{2.0, 0.0}) && (numbers_of(b, "a").data == Numbers{1.0, 1.0}) && (numbers_of(b, "b").data == Numbers{0.0, 2.0}));
    try { df.unstack("flag", "s", "v"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::OperationFailed); }
    const auto u = df.unstack("flag", "i", "v");            // the last row of a pair wins; NaN where there is none
    CHECK((u.column_names == Strings{"flag", "-2", "10", "9", "NaN"}));
    CHECK(numbers_of(u, "10").data[0] == 6.0 && numbers_of(u, "10").data[1] == 3.0 && std::isnan(numbers_of(u, "-2").data[1]) && numbers_of(u, "NaN").data[1] == 5.0);
    const auto d = df.crosstab("s", "s");                   // a column against itself: the diagonal
    CHECK((d.column_names == Strings{"s", "", "a", "b"}) && (numbers_of(d, "").data == Numbers{2.0, 0.0, 0.0}) && (numbers_of(d, "b").data == Numbers{0.0, 0.0, 2.0}));
}

static void test_label_equal_to_the_index_name_and_resident_columns() {
    OptimizedDataFrame df;
    df.add_column("k", StringColumn({"p", "q", "p"}));
    df.add_column("c", StringColumn({"k", "z", "z"}));
    df.add_column("v", Float64Column({1.0, 2.0, 3.0}));
    try { df.crosstab("k", "c"); CHECK(false); } catch (const Error &e) { CHECK(e.kind == Error::DuplicateColumnName); }
    auto r = sales();
    r.make_resident();
    const auto s = r.pivot_table("category", "region", "sales", AggFunction::Sum);
    CHECK((numbers_of(s, "East").data == Numbers{150.0, 250.0, 300.0}));
    const auto c = r.crosstab("region", "flag");
    CHECK((strings_of(c, "region") == Strings{"East", "North", "West"}) && (numbers_of(c, "true").data == Numbers{2.0, 1.0, 1.0}));
}

int main() {
    RUN(test_errors_before_any_device_call);
    int32_t n_dev = 0;
    if (pandrs_hip_init(nullptr) != PANDRS_HIP_OK || pandrs_hip_device_count(&n_dev) != PANDRS_HIP_OK || n_dev == 0) {
        std::printf("%d tests, %d failed checks\n", g_run, g_failed);
        std::fprintf(stderr, "no HIP device available: %s\n", pandrs_hip_last_error());
        return g_failed ? 2 : 1;
    }
    RUN(test_crosstab);
    RUN(test_unstack);
    RUN(test_pivot);
    RUN(test_pivot_table);
    RUN(test_other_key_types_and_missing_cells);
    RUN(test_label_equal_to_the_index_name_and_resident_columns);
    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 2 : 0;
}
