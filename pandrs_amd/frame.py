"""Host-side mirror of the reference's interface for the hot path — same names, argument meaning and
error behaviour — so the parity tests read like the reference's own tests.

  reference (file:line)                                               here
  OptimizedDataFrame  src/optimized/split_dataframe/core.rs:14-25     OptimizedDataFrame
  Int64Column ...     src/column/*.rs                                 Int64Column / Float64Column / StringColumn / BooleanColumn
  GLOBAL_STRING_POOL  src/column/string_pool.rs:6-53                  GLOBAL_STRING_POOL
  group_by            src/optimized/split_dataframe/group/grouping.rs:22      OptimizedDataFrame.group_by
  GroupBy.aggregate   src/optimized/split_dataframe/group/aggregation.rs:763  GroupBy.aggregate
  sum/mean/../agg     src/optimized/split_dataframe/group/operations.rs:438-521  GroupBy.sum ... GroupBy.agg
  *_join / join_impl  src/optimized/split_dataframe/join.rs:32-555    OptimizedDataFrame.inner_join ...
  sort_by / sort_by_columns  src/optimized/split_dataframe/sort.rs:18-272  OptimizedDataFrame.sort_by / sort_by_columns
  select / filter     src/optimized/split_dataframe/data_ops.rs:15-121    OptimizedDataFrame.select / filter
  filter_rows         src/optimized/split_dataframe/row_ops.rs:26-130     OptimizedDataFrame.filter_rows
  par_filter          src/optimized/split_dataframe/parallel.rs:21-230    OptimizedDataFrame.par_filter
  select_by_mask      src/optimized/split_dataframe/select.rs:150-167     OptimizedDataFrame.select_by_mask
  rolling / expanding / ewm  src/dataframe/window.rs:13-160 over src/series/window.rs  OptimizedDataFrame.rolling / ...
  LazyFrame           src/optimized/lazy.rs:98-170, :186-425          LazyFrame
  AggregateOp         src/optimized/split_dataframe/group/types.rs:11-34   AggregateOp
  JoinType            src/optimized/split_dataframe/join.rs:11-20     JoinType

This is what the Rust call-outs of INTEGRATION.md §3 do: adapt columns to the C ABI, call the
device engine, stringify group keys, name result columns.  All arithmetic happens in
libpandrs_hip.so; there is no CPU implementation of groupby or join here.
"""
import math
from decimal import Decimal
from enum import IntEnum

import numpy as np

from . import _lib as L
from .engine import Context, PandrsHipError, ColumnTypeMismatch, OperationFailed, EmptyError


class AggregateOp(IntEnum):          # types.rs:11-34, same order
    Sum = 0
    Mean = 1
    Min = 2
    Max = 3
    Count = 4
    Std = 5
    Var = 6
    Median = 7
    First = 8
    Last = 9
    Custom = 10
    Nunique = 11                     # not in the reference's enum: the legacy AggFunc::Nunique (src/dataframe/groupby.rs:41)


class RankMethod(IntEnum):           # pandas_compat/types.rs:48-59, same order
    Average = 0
    Min = 1
    Max = 2
    First = 3
    Dense = 4


class AggFunction(IntEnum):          # pivot/mod.rs:12-23, same order
    Sum = 0
    Mean = 1
    Min = 2
    Max = 3
    Count = 4

    def name(self):                  # pivot/mod.rs:27-35
        return self._name_.lower()

    @classmethod
    def from_str(cls, s):            # pivot/mod.rs:38-47: None for a name it does not know
        return {"sum": cls.Sum, "mean": cls.Mean, "avg": cls.Mean, "average": cls.Mean, "min": cls.Min, "minimum": cls.Min,
                "max": cls.Max, "maximum": cls.Max, "count": cls.Count}.get(str(s).lower())


class JoinType(IntEnum):             # join.rs:11-20
    Inner = 0
    Left = 1
    Right = 2
    Outer = 3


class ColumnNotFound(KeyError):      # Error::ColumnNotFound (grouping.rs:55, join.rs:87)
    pass


class EmptyColumnList(ValueError):    # Error::EmptyColumnList (split_dataframe/sort.rs:147-149)
    pass


class InconsistentArrayLengths(ValueError):   # Error::InconsistentArrayLengths { expected, found } (sort.rs:161-166)
    def __init__(self, expected, found):
        super().__init__("Inconsistent array lengths: expected %d, found %d" % (expected, found))
        self.expected, self.found = expected, found


class FormatError(ValueError):        # Error::Format (select.rs:151-157: a mask whose length is not the row count)
    pass


class InvalidValue(ValueError):       # Error::InvalidValue (series/window.rs:113-116, :567-573, dataframe/window.rs:62-67)
    pass


class DuplicateColumnName(ValueError):
    pass


class InconsistentRowCount(ValueError):
    pass


_OP_NAME = {AggregateOp.Sum: "sum", AggregateOp.Mean: "mean", AggregateOp.Min: "min", AggregateOp.Max: "max",
            AggregateOp.Count: "count", AggregateOp.Std: "std", AggregateOp.Var: "var",
            AggregateOp.Median: "median", AggregateOp.First: "first", AggregateOp.Last: "last",
            AggregateOp.Custom: "custom", AggregateOp.Nunique: "nunique"}       # operations.rs:501-514


# ---------------------------------------------------------------------------------------------- columns
class StringPool:
    """Process-global string pool: equal string <=> equal u32 code (string_pool.rs:28-53)."""

    def __init__(self):
        self._code = {}
        self._strings = []

    def get_or_insert(self, s):
        c = self._code.get(s)
        if c is None:
            c = len(self._strings)
            self._code[s] = c
            self._strings.append(s)
        return c

    def get(self, code):
        return self._strings[code]

    def find(self, s):
        """The code of a string the pool already holds, None for one it has never seen (nothing is inserted)."""
        return self._code.get(s)

    def rank_table(self):
        """rank[code] = position of the code's string in byte-wise order (Rust String: Ord).  UTF-8 byte order and
        code-point order (Python str comparison) are the same order."""
        order = sorted(range(len(self._strings)), key=self._strings.__getitem__)
        rank = np.empty(len(order), np.uint32)
        rank[np.asarray(order, dtype=np.int64)] = np.arange(len(order), dtype=np.uint32)
        return rank

    def __len__(self):
        return len(self._strings)


GLOBAL_STRING_POOL = StringPool()


def create_bitmask(nulls):
    """bool list -> LSB-first bitmap, 1 = null (src/core/column.rs:163-177)."""
    return np.packbits(np.asarray(nulls, dtype=bool), bitorder="little")


class _Column:
    dtype = None
    type_name = None

    def __init__(self, data, null_mask, length):
        self.data = data
        self.null_mask = null_mask
        self.length = length

    def len(self):
        return self.length

    def __len__(self):
        return self.length

    def column_type(self):
        return self.type_name

    def is_null(self, i):
        return self.null_mask is not None and bool((self.null_mask[i >> 3] >> (i & 7)) & 1)

    def view(self):
        """(data, null_mask, dtype) triple for the engine."""
        return (self.data, self.null_mask, self.dtype)

    @staticmethod
    def _mask(nulls):
        if nulls is None or not np.any(nulls):
            return None
        return create_bitmask(nulls)


class _NumericColumn(_Column):
    """The null-skipping column folds of src/column/{int64,float64}_column.rs:100-199 on the device
    (pandrs_hip_reduce_stats): None exactly where the reference returns None."""

    def _stats(self):
        return get_context().column_stats(self.view(), self.length)

    def sum(self):
        if self.length == 0:
            return 0 if self.dtype == L.I64 else 0.0
        st = self._stats()
        return int(st["sum_i64"]) if self.dtype == L.I64 else float(st["sum_f64"])

    def mean(self):
        if self.length == 0:
            return None
        st = self._stats()
        if st["count"] == 0:
            return None
        return (float(st["sum_i64"]) if self.dtype == L.I64 else st["sum_f64"]) / st["count"]

    def _extreme(self, which):
        if self.length == 0:
            return None
        st = self._stats()
        if self.dtype == L.I64:
            return None if st["count"] == 0 else int(st[which + "_i64"])
        return None if st["count_finite"] == 0 else float(st[which + "_finite"])      # non-finite values are skipped

    def min(self):
        return self._extreme("min")

    def max(self):
        return self._extreme("max")


class Int64Column(_NumericColumn):   # src/column/int64_column.rs:52-66
    dtype, type_name = L.I64, "Int64"

    def __init__(self, data, nulls=None):
        data = np.ascontiguousarray(data, dtype=np.int64)
        super().__init__(data, self._mask(nulls), len(data))

    @classmethod
    def with_nulls(cls, data, nulls):
        return cls(data, nulls)

    def get(self, i):
        return None if self.is_null(i) else int(self.data[i])


class Float64Column(_NumericColumn): # src/column/float64_column.rs:9-13
    dtype, type_name = L.F64, "Float64"

    def __init__(self, data, nulls=None):
        data = np.ascontiguousarray(data, dtype=np.float64)
        super().__init__(data, self._mask(nulls), len(data))

    @classmethod
    def with_nulls(cls, data, nulls):
        return cls(data, nulls)

    def get(self, i):
        return None if self.is_null(i) else float(self.data[i])


class StringColumn(_Column):         # src/column/string_column.rs:26-72 (GlobalPool mode)
    dtype, type_name = L.U32CODE, "String"

    def __init__(self, values, nulls=None, _codes=None):
        if _codes is None:
            _codes = np.fromiter((GLOBAL_STRING_POOL.get_or_insert(s) for s in values), dtype=np.uint32,
                                 count=len(values))
        super().__init__(np.ascontiguousarray(_codes, dtype=np.uint32), self._mask(nulls), len(_codes))

    @classmethod
    def with_nulls(cls, values, nulls):
        return cls(values, nulls)

    @classmethod
    def from_codes(cls, codes, null_mask=None):
        c = cls([], _codes=codes)
        c.null_mask = null_mask
        return c

    def get(self, i):
        return None if self.is_null(i) else GLOBAL_STRING_POOL.get(int(self.data[i]))

    def to_list(self):
        return [self.get(i) for i in range(self.length)]


class BooleanColumn(_Column):        # src/column/boolean_column.rs:10-15 (bit-packed)
    dtype, type_name = L.BOOLBITS, "Boolean"

    def __init__(self, data, nulls=None, _bits=None, _length=None):
        if _bits is None:
            data = np.asarray(data, dtype=bool)
            _bits, _length = np.packbits(data, bitorder="little"), len(data)
        super().__init__(_bits, self._mask(nulls), _length)

    @classmethod
    def with_nulls(cls, data, nulls):
        return cls(data, nulls)

    def get(self, i):
        return None if self.is_null(i) else bool((self.data[i >> 3] >> (i & 7)) & 1)


def rust_f64_to_string(v):
    """f64::to_string(): shortest round-trip digits, never an exponent ("1", "0.1", "NaN", "inf", "-0")."""
    if v != v:
        return "NaN"
    if v in (float("inf"), float("-inf")):
        return "inf" if v > 0 else "-inf"
    s = format(Decimal(repr(float(v))), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    if s in ("0", "-0"):
        return "-0" if np.signbit(v) else "0"
    return s


def _key_strings(dtype, cells, nulls, null_string="NULL"):
    """Group-key cells -> the strings the reference's result frame holds (grouping.rs:69-98)."""
    out = []
    for cell, nul in zip(cells.tolist(), nulls.tolist()):
        if nul:
            out.append(null_string)
        elif dtype == L.I64:
            out.append(str(int(np.int64(np.uint64(cell)))))
        elif dtype == L.F64:
            out.append(rust_f64_to_string(float(np.uint64(cell).view(np.float64))))
        elif dtype == L.U32CODE:
            out.append(GLOBAL_STRING_POOL.get(int(cell)))
        else:
            out.append("true" if cell else "false")
    return out


# ---------------------------------------------------------------------------------------------- f64 arithmetic as Rust does it
_F64_EPSILON = 2.0 ** -52          # f64::EPSILON


def _fdiv(a, b):
    """a / b by IEEE rules (Python raises on a zero divisor)."""
    if b == 0.0:
        if a == 0.0 or math.isnan(a):
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _fsqrt(x):
    """f64::sqrt: NaN for a negative or NaN operand (math.sqrt raises on the former)."""
    return math.nan if math.isnan(x) or x < 0.0 else math.sqrt(x)


def _fexp(x):
    """f64::exp: +inf past the range (math.exp raises)."""
    return math.inf if x > 709.782712893384 else math.exp(x)


# ---------------------------------------------------------------------------------------------- context
_default_ctx = None


def get_context():
    """Lazily created process-wide engine context (cf. get_gpu_manager, src/gpu/mod.rs:249-282)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# StatDescribe's keys in stats_list order (stats.rs:74-83) and the pandrs_hip_describe_stats field behind each
_DESCRIBE_FIELDS = (("count", "count"), ("mean", "mean"), ("std", "std"), ("min", "min"), ("25%", "q1"), ("50%", "median"),
                    ("75%", "q3"), ("max", "max"))


class StatDescribe:                   # src/optimized/split_dataframe/stats.rs:13-19
    def __init__(self, stats_list):
        self.stats_list = list(stats_list)        # ordered (name, value) pairs
        self.stats = dict(self.stats_list)

    def __repr__(self):
        return "StatDescribe(%r)" % (self.stats_list,)


_WINDOW_OPS = {"sum": L.WINDOW_SUM, "mean": L.WINDOW_MEAN, "var": L.WINDOW_VAR, "std": L.WINDOW_STD, "min": L.WINDOW_MIN,
               "max": L.WINDOW_MAX, "count": L.WINDOW_COUNT}
_ROLLING_OPS = set(_WINDOW_OPS.values())
_EWM_OPS = {L.WINDOW_MEAN, L.WINDOW_STD, L.WINDOW_VAR}


# ---------------------------------------------------------------------------------------------- frame
class OptimizedDataFrame:
    def __init__(self):
        self.columns = []
        self.column_names = []
        self.column_indices = {}
        self._row_count = 0
        self.multi_index = None           # list of key tuples when a multi-key group_by built a multi-index
        self.multi_index_names = None

    # -- construction / inspection (core.rs) ----------------------------------------------------------
    def add_column(self, name, column):
        if name in self.column_indices:
            raise DuplicateColumnName(name)
        if self.columns and column.len() != self._row_count:
            raise InconsistentRowCount("expected %d rows, found %d" % (self._row_count, column.len()))
        self.column_indices[name] = len(self.columns)
        self.column_names.append(name)
        self.columns.append(column)
        self._row_count = column.len()
        return self

    def column(self, name):
        if name not in self.column_indices:
            raise ColumnNotFound(name)
        return self.columns[self.column_indices[name]]

    def contains_column(self, name):
        return name in self.column_indices

    def row_count(self):
        return self._row_count

    def column_count(self):
        return len(self.columns)

    # -- groupby (grouping.rs:22-115) -------------------------------------------------------------------
    def group_by(self, columns):
        return self.group_by_with_options(columns, True)      # grouping.rs:22-28

    def group_by_with_options(self, columns, as_multi_index):
        columns = [columns] if isinstance(columns, str) else list(columns)
        for c in columns:
            if c not in self.column_indices:
                raise ColumnNotFound(c)                       # grouping.rs:53-57
        return GroupBy(self, columns, as_multi_index and len(columns) > 1)   # grouping.rs:107

    def par_groupby(self, group_by_columns):
        """par_groupby (grouping.rs:124-331): {joined key -> sub-frame}.  Keys are the parts joined
        with "_" (:186), a null part is "NA" (:158); tuples that collide after joining share a
        group, as in the reference.  The row lists come from the device (groupby_indices), every
        sub-frame is a device gather of all columns (:286-328)."""
        cols = [group_by_columns] if isinstance(group_by_columns, str) else list(group_by_columns)
        for c in cols:
            if c not in self.column_indices:
                raise ColumnNotFound(c)
        gb = GroupBy(self, cols, False)
        merged = {}
        for key, rows in gb._group_rows(null_string="NA").items():
            name = "_".join(key)
            if name in merged:
                merged[name] = np.sort(np.concatenate([merged[name], rows]))
            else:
                merged[name] = rows
        return {name: self.filter_by_indices(rows) for name, rows in merged.items()}

    def filter_by_indices(self, indices):
        """data_ops.rs:124-209: row gather of every column; nulls become 0 / 0.0 / "" / false and the
        result carries no masks; out-of-range indices are dropped."""
        idx = np.asarray(indices, dtype=np.int64)
        idx = idx[(idx >= 0) & (idx < self._row_count)]
        result = OptimizedDataFrame()
        if not self.columns:
            return result
        g = _Gatherer(get_context(), idx, idx)
        for name in self.column_names:
            result.add_column(name, g.take(self.column(name), left=True))
        return result

    # -- sort (split_dataframe/sort.rs:18-272) --------------------------------------------------------------
    def sort_by(self, by, ascending):
        """sort.rs:18-143: the frame with its rows ordered by one column; see sort_by_columns."""
        return self.sort_by_columns([by], [ascending])

    def sort_by_columns(self, by, ascending=None):
        """sort.rs:146-272: rows ordered by by[0], then by[1], ... (ascending: one flag per column, None = all
        ascending).  Stable, also descending; nulls last in both directions; -0.0 ties 0.0; strings in byte-wise
        order; NaN after every number and before nulls (the reference's NaN order is unspecified: pandrs_hip.h).
        The result is select_rows_by_indices_impl's (select.rs:172-226): nulls become 0 / 0.0 / "" / false, no
        null masks, and an empty frame has no columns.  The columns keep this frame's order (the reference emits
        them in HashMap order, which is unspecified)."""
        by = [by] if isinstance(by, str) else list(by)
        if not by:
            raise EmptyColumnList("empty column list")                      # sort.rs:147-149
        for name in by:
            if name not in self.column_indices:
                raise ColumnNotFound(name)                                  # sort.rs:152-156
        if ascending is not None and len(ascending) != len(by):
            raise InconsistentArrayLengths(len(by), len(ascending))         # sort.rs:159-167
        result = OptimizedDataFrame()
        if self._row_count == 0:
            return result                                                   # select.rs:177-179
        cols = [self.column(name) for name in by]
        rank = GLOBAL_STRING_POOL.rank_table() if any(c.dtype == L.U32CODE for c in cols) else None
        ctx = get_context()
        idx = ctx.sort_indices([c.view() for c in cols], self._row_count, ascending, rank)
        g = _Gatherer(ctx, idx, idx)
        for name in self.column_names:
            result.add_column(name, g.take(self.column(name), left=True))
        return result

    # -- select / filter (data_ops.rs:15-121, row_ops.rs:26-130, parallel.rs:21-230, select.rs:150-167) ----------
    def select(self, columns):
        """data_ops.rs:15-34: a frame of the named columns, in the order given, shared as they are (null masks kept).
        A missing name is ColumnNotFound; a repeated one DuplicateColumnName (add_column).  Host only."""
        result = OptimizedDataFrame()
        for name in ([columns] if isinstance(columns, str) else columns):
            result.add_column(name, self.column(name))
        return result

    def _condition(self, condition_column):
        if condition_column not in self.column_indices:
            raise ColumnNotFound(condition_column)                       # data_ops.rs:39-42
        cond = self.column(condition_column)
        if cond.dtype != L.BOOLBITS:                                     # data_ops.rs:115-119
            raise ColumnTypeMismatch(L.ERR_TYPE_MISMATCH, "Column type mismatch: column '%s' expected Boolean, found %s"
                                     % (condition_column, cond.column_type()))
        return cond

    def _compact(self, cond_view):
        """Every column compacted on the device through one selection (pandrs_hip_filter_indices, then
        pandrs_hip_filter_gather per column): nulls become 0 / 0.0 / "" / false, no masks.  -> (frame, count)."""
        ctx = get_context()
        _, count = ctx.filter_indices(cond_view, self._row_count, indices=False)
        result = OptimizedDataFrame()
        for name in self.column_names:
            col = self.column(name)
            fill = GLOBAL_STRING_POOL.get_or_insert("") if col.dtype == L.U32CODE else 0
            result.add_column(name, _Gatherer._wrap(col, ctx.filter_gather(col.view(), self._row_count, count, fill)))
        return result, count

    def filter(self, condition_column):
        """data_ops.rs:37-121: the rows whose Boolean condition is Some(true), in order (a null condition drops the row).
        Every column is kept; nulls become 0 / 0.0 / "" / false and the result has no masks.  No selected row: every
        column with 0 rows.  A missing column is ColumnNotFound, a non-Boolean one ColumnTypeMismatch."""
        cond = self._condition(condition_column)
        if self._row_count == 0:
            return self._empty_columns()
        return self._compact(cond.view())[0]

    def filter_rows(self, condition_column):
        """row_ops.rs:26-130: filter's body again (the same rows, defaults and empty shape; the frame has no index here)."""
        return self.filter(condition_column)

    def par_filter(self, condition_column):
        """parallel.rs:21-230: the same rows as filter.  No selected row: explicitly empty typed columns, one per column
        (parallel.rs:73-90), which is filter's shape too.  The reference's serial / parallel split (100 000 rows)
        changes only how the host loops run; here every size takes the device."""
        cond = self._condition(condition_column)
        if self._row_count == 0:
            return self._empty_columns()
        result, count = self._compact(cond.view())
        return result if count else self._empty_columns()

    def select_by_mask(self, mask):
        """select.rs:150-167: the rows where mask is true, through select_rows_by_indices_impl (select.rs:172-226):
        nulls become defaults, no masks, and no selected row is a frame with NO columns.  A mask whose length is not the
        row count is Error::Format (FormatError).  The mask is packed to bits and filtered on the device.  The columns
        keep this frame's order (the reference emits them in HashMap order, which is unspecified)."""
        mask = np.asarray(mask, dtype=bool).reshape(-1)
        if mask.shape[0] != self._row_count:
            raise FormatError("Mask length (%d) does not match DataFrame row count (%d)" % (mask.shape[0], self._row_count))
        if self._row_count == 0 or not self.columns:
            return OptimizedDataFrame()                                  # select.rs:177-179
        result, count = self._compact((np.packbits(mask, bitorder="little"), None, L.BOOLBITS))
        return result if count else OptimizedDataFrame()

    def _empty_columns(self):
        result = OptimizedDataFrame()
        for name in self.column_names:
            result.add_column(name, _empty_like(self.column(name)))
        return result

    # -- window statistics (dataframe/window.rs:13-160 over series/window.rs) -------------------------------------
    def _window_column(self, column_name):
        if column_name not in self.column_indices:
            raise ColumnNotFound(column_name)
        col = self.column(column_name)
        if col.dtype not in (L.I64, L.F64):
            raise ColumnTypeMismatch(L.ERR_TYPE_MISMATCH, "Column type mismatch: column '%s' expected Int64 or Float64, found %s"
                                     % (column_name, col.column_type()))
        return col

    @staticmethod
    def _window_op(kind_name, operation, allowed):
        op = _WINDOW_OPS.get(str(operation).lower())                    # window.rs:54: to_lowercase
        if op is None or op not in allowed:
            raise InvalidValue("Unsupported %s operation: %s" % (kind_name, operation))
        return op

    def _with_window(self, col, column_name, operation, new_column_name, kind, op, **spec):
        """A new frame: every column of this one, then a Float64Column named new_column_name or "{column}_{operation}"
        (window.rs:72), n rows, no null mask (NaN marks a None)."""
        name = new_column_name if new_column_name is not None else "%s_%s" % (column_name, operation)
        if name in self.column_indices:
            raise DuplicateColumnName(name)
        n = self._row_count
        values = get_context().window(col.view(), n, kind, op, out_device=False, **spec) if n else np.empty(0)
        result = OptimizedDataFrame()
        for c in self.column_names:
            result.add_column(c, self.column(c))
        result.add_column(name, Float64Column(values))
        return result

    def rolling(self, window_size, column_name, operation, new_column_name=None, *, min_periods=None, center=False, ddof=1):
        """DataFrameWindowExt::rolling (dataframe/window.rs:45-79; Rolling, series/window.rs:107-345): row i's window is
        [max(0, i+1-w), i+1), or with center start = i >= w/2 ? i - w/2 : 0, end = min(start+w, n).  operation: sum,
        mean, var, std (ddof), min, max, count, any case.  min_periods defaults to window_size.  Errors, all before any
        device call: ColumnNotFound, ColumnTypeMismatch (not Int64 / Float64), InvalidValue (window_size 0, an unknown
        operation, median / quantile), DuplicateColumnName.  The string dispatch takes no "median" / "quantile", as the
        reference's (window.rs:54-67): they live in rolling_median and apply_rolling(config).median() / .quantile(q)."""
        col = self._window_column(column_name)
        if int(window_size) <= 0:
            raise InvalidValue("Window size must be greater than 0")            # series/window.rs:112-117
        if min_periods is not None and int(min_periods) < 0:
            raise InvalidValue("min_periods must be >= 0")
        if int(ddof) < 0:
            raise InvalidValue("ddof must be >= 0")
        op = self._window_op("rolling", operation, _ROLLING_OPS)
        return self._with_window(col, column_name, operation, new_column_name, L.WINDOW_KIND_ROLLING, op, window=int(window_size),
                                 min_periods=-1 if min_periods is None else int(min_periods), center=bool(center), ddof=int(ddof))

    def expanding(self, min_periods, column_name, operation, new_column_name=None, *, ddof=1):
        """DataFrameWindowExt::expanding (dataframe/window.rs:82-119; Expanding, series/window.rs:379-500): row i's
        window is [0, i+1); min_periods as given (0 allowed).  Same operations and errors as rolling; the expanding
        median and quantile live in apply_expanding(config).median() / .quantile(q)."""
        col = self._window_column(column_name)
        if int(min_periods) < 0:
            raise InvalidValue("min_periods must be >= 0")
        if int(ddof) < 0:
            raise InvalidValue("ddof must be >= 0")
        op = self._window_op("expanding", operation, _ROLLING_OPS)
        return self._with_window(col, column_name, operation, new_column_name, L.WINDOW_KIND_EXPANDING, op,
                                 min_periods=int(min_periods), ddof=int(ddof))

    def ewm(self, column_name, operation, span=None, alpha=None, new_column_name=None, *, halflife=None):
        """DataFrameWindowExt::ewm (dataframe/window.rs:122-160; EWM, series/window.rs:549-724).  alpha = 2/(span+1)
        when span is given, else alpha (validated to (0, 1], :567-573), else 1 - exp(-ln2/halflife) (get_alpha, :608);
        none of them is InvalidValue.  operation: mean, std, var (var = the std output squared, :715-724)."""
        col = self._window_column(column_name)
        if span is not None:
            if int(span) < 0:
                raise InvalidValue("span must be >= 0")
            a = 2.0 / (float(int(span)) + 1.0)
        elif alpha is not None:
            a = float(alpha)
            if not (0.0 < a <= 1.0):
                raise InvalidValue("Alpha must be between 0 and 1")
        elif halflife is not None:
            with np.errstate(divide="ignore", over="ignore"):
                a = float(1.0 - np.exp(-math.log(2.0) / np.float64(halflife)))
        else:
            raise InvalidValue("Must specify either span or alpha for EWM")
        if not math.isfinite(a):
            raise InvalidValue("EWM alpha %r is not finite" % a)
        op = self._window_op("EWM", operation, _EWM_OPS)
        return self._with_window(col, column_name, operation, new_column_name, L.WINDOW_KIND_EWM, op, alpha=a)

    # -- window order statistics (pandas_compat/helpers/window_ops.rs:206-240; dataframe/enhanced_window.rs) ------------
    def rolling_median(self, column, window, min_periods=None):
        """PandasCompatExt::rolling_median (pandas_compat/functions.rs:2055 over helpers/window_ops.rs:206-240): the
        median of the trailing window's non-null, non-NaN cells, NaN where fewer than min_periods (default: window) of
        them, or none, are there.  window 0 acts as 1 (the reference's saturating_sub).  -> a float64 numpy array.
        Errors, before any device call: ColumnNotFound, ColumnTypeMismatch."""
        col = self._window_column(column)
        if int(window) < 0 or (min_periods is not None and int(min_periods) < 0):
            raise InvalidValue("window and min_periods must be >= 0")          # (usize in the reference)
        n = self._row_count
        if n == 0:
            return np.empty(0)
        mp = int(window) if min_periods is None else int(min_periods)
        return get_context().window_quantile(col.view(), n, L.WINDOW_KIND_ROLLING, median=True, window=max(int(window), 1),
                                             min_periods=mp, nan_missing=True, out_device=False)

    def apply_rolling(self, config):
        """DataFrameWindowExt::apply_rolling (dataframe/enhanced_window.rs:204-209): the operations of a DataFrameRolling
        configuration over this frame."""
        return DataFrameRollingOps(self, config)

    def apply_expanding(self, config):
        """DataFrameWindowExt::apply_expanding (dataframe/enhanced_window.rs:211-216)."""
        return DataFrameExpandingOps(self, config)

    # -- whole-column reductions (K1: split_dataframe/aggregate.rs:21-215) ----------------------------------
    def _stats(self, name):
        col = self.column(name)
        if col.dtype not in (L.I64, L.F64):        # Error::Type (aggregate.rs:57)
            raise ColumnTypeMismatch(L.ERR_TYPE_MISMATCH, "Column '%s' is not a numeric type" % name)
        return get_context().column_stats(col.view(), col.len())

    def sum(self, name):
        """aggregate.rs:21-62: the non-null values as f64 (`v as f64` for Int64), 0.0 when there is none."""
        return float(self._stats(name)["sum_f64"])

    def mean(self, name):
        st = self._stats(name)
        if st["count"] == 0:                       # aggregate.rs:87, :99
            raise EmptyError(L.ERR_OPERATION_FAILED, "Column '%s' is empty" % name)
        return float(st["sum_f64"]) / st["count"]

    def min(self, name):
        st = self._stats(name)
        if st["count"] == 0:                       # aggregate.rs:185, :198
            raise EmptyError(L.ERR_OPERATION_FAILED, "Column '%s' is empty" % name)
        return float(st["min"])                    # fold(+inf, f64::min): NaN dropped, infinities kept

    def max(self, name):
        st = self._stats(name)
        if st["count"] == 0:                       # aggregate.rs:135, :148
            raise EmptyError(L.ERR_OPERATION_FAILED, "Column '%s' is empty" % name)
        return float(st["max"])

    # -- describe (split_dataframe/stats.rs:50-171 over stats/descriptive.rs:91-200) ---------------------------
    def describe(self, column_name):
        """OptimizedDataFrame::describe (stats.rs:50-151): count, mean, std (two passes, count - 1), min, the 25 / 50 / 75
        percentiles (linear interpolation at (p / 100) * (count - 1)) and max of the non-null cells of an Int64
        (`v as f64`) or Float64 column, from one device call (pandrs_hip_describe: a radix select, no sort).  ->
        StatDescribe.  Errors before any device call: ColumnNotFound, ColumnTypeMismatch for Error::Type (a String or
        Boolean column, as sum()).  InvalidValue for a column without a non-null cell (descriptive.rs:92-96) and for one
        with a single non-null cell (the reference's confidence interval refuses 0 degrees of freedom,
        stats/distributions.rs:188-193).  NaN cells order after every number (pandrs_hip.h)."""
        col = self.column(column_name)
        if col.dtype not in (L.I64, L.F64):        # Error::Type (stats.rs:146-149)
            raise ColumnTypeMismatch(L.ERR_TYPE_MISMATCH, "Column '%s' is not a numeric type" % column_name)
        st = get_context().describe(col.view(), col.len()) if col.len() else {"count": 0}
        if st["count"] == 0:
            raise InvalidValue("Cannot compute statistics for empty data")
        if st["count"] == 1:
            raise InvalidValue("Degrees of freedom must be positive")
        return StatDescribe([(key, float(st[field])) for key, field in _DESCRIBE_FIELDS])

    def describe_all(self):
        """OptimizedDataFrame::describe_all (stats.rs:157-171): {column name -> StatDescribe} of every Int64 / Float64
        column; a column whose describe fails (no non-null cell) is left out."""
        results = {}
        for name in self.column_names:
            if self.column(name).dtype in (L.I64, L.F64):
                try:
                    results[name] = self.describe(name)
                except InvalidValue:                # stats.rs:164: `if let Ok(desc)`; a device failure is still raised
                    pass
        return results

    # -- rank (dataframe/pandas_compat/functions.rs:193-236) ----------------------------------------------------
    def rank(self, column_name, method=RankMethod.Average):
        """PandasCompatExt::rank (functions.rs:193-236): the ascending 1-based rank of every row of an Int64 or Float64
        column, from one device call (pandrs_hip_rank: the stable radix sort, tie-run boundaries, a scatter).  A tie run
        at sorted positions [s, e) ranks (s + e + 1) / 2 (Average), s + 1 (Min), e (Max), position + 1 in row order
        (First) or the run's number (Dense).  -> float64 numpy array of row_count() ranks (the reference's Vec<f64>).
        Errors before any device call: ColumnNotFound, ColumnTypeMismatch for a String or Boolean column (as describe).
        Deviations (pandrs_hip.h): a NaN or null cell gets NaN and takes no rank (the reference loops forever on NaN and
        returns InvalidValue on a missing value); Int64 cells are compared as integers, not as f64."""
        col = self.column(column_name)
        if col.dtype not in (L.I64, L.F64):
            raise ColumnTypeMismatch(L.ERR_TYPE_MISMATCH, "Column '%s' is not a numeric type" % column_name)
        method = RankMethod(method)
        if col.len() == 0:
            return np.empty(0, np.float64)
        return np.asarray(get_context().rank(col.view(), col.len(), int(method), out_device=False), dtype=np.float64)

    # -- nlargest / nsmallest / idxmax / idxmin (dataframe/pandas_compat/functions.rs:159-192) --------------------
    def _numeric(self, column_name):
        col = self.column(column_name)
        if col.dtype not in (L.I64, L.F64):
            raise ColumnTypeMismatch(L.ERR_TYPE_MISMATCH, "Column '%s' is not a numeric type" % column_name)
        return col

    def _topk(self, n, column_name, largest):
        """One pandrs_hip_topk call -> the frame of those rows, assembled as sort_by_columns assembles its own
        (select_rows_by_indices: nulls become 0 / 0.0 / "" / false, no masks, no columns when there are no rows)."""
        col = self._numeric(column_name)
        n = int(n)
        if n < 0:
            raise InvalidValue("n must not be negative, got %d" % n)
        result = OptimizedDataFrame()
        if self._row_count == 0 or n == 0:
            return result
        ctx = get_context()
        idx, _ = ctx.topk(col.view(), self._row_count, n, largest, out_device=True)
        g = _Gatherer(ctx, idx, idx)
        for name in self.column_names:
            result.add_column(name, g.take(self.column(name), left=True))
        return result

    def nlargest(self, n, column):
        """PandasCompatExt::nlargest (functions.rs:159-166): the min(n, row_count()) rows with the largest values of an
        Int64 or Float64 column, largest first, ties in row order, from one device call (pandrs_hip_topk: a radix select,
        a compaction, a sort of fewer than n rows) - sort_by(column, False)'s first n rows without the sort.  Errors before
        any device call: ColumnNotFound, ColumnTypeMismatch for a String or Boolean column (as rank).  Deviations
        (pandrs_hip.h): NaN rows, then null rows, come after every number (the reference's order with a NaN present is
        unspecified); Int64 cells are compared as integers."""
        return self._topk(n, column, True)

    def nsmallest(self, n, column):
        """PandasCompatExt::nsmallest (functions.rs:167-174): as nlargest, smallest first; NaN and null rows still last."""
        return self._topk(n, column, False)

    def _idx_extreme(self, column_name, which):
        col = self._numeric(column_name)
        if col.len() == 0:
            return None
        rows = get_context().arg_extreme(col.view(), col.len())
        return None if rows is None else rows[which]

    def idxmax(self, column):
        """PandasCompatExt::idxmax (functions.rs:175-183): the row of the largest value, the LAST one among equals
        (Iterator::max_by), NaN and null cells skipped; None when the column holds no number.  One device pass."""
        return self._idx_extreme(column, 1)

    def idxmin(self, column):
        """PandasCompatExt::idxmin (functions.rs:184-192): the row of the smallest value, the FIRST one among equals
        (Iterator::min_by), NaN and null cells skipped; None when the column holds no number.  One device pass."""
        return self._idx_extreme(column, 0)

    # -- shape statistics (dataframe/pandas_compat/functions.rs:1617-1665, helpers/aggregations.rs:8-225) ----------------
    # Every method: one pandrs_hip_moments call (two streams at the most over the column, whatever it asks for) and/or one
    # pandrs_hip_order_stats call, then the reference's expression on the host over the returned fields.  The cells that count
    # are neither null nor NaN.  Errors before any device call: ColumnNotFound, ColumnTypeMismatch for a String or Boolean column.
    def _moments(self, column, want):
        c = self._numeric(column)
        return get_context().moments([c.view()], c.len(), want)[0]

    def _order_stats(self, column, ops):
        c = self._numeric(column)
        return get_context().order_stats(c.view(), c.len(), ops)

    def skew(self, column):
        """skew (functions.rs:1617-1640): NaN below 3 valid cells (:1621) and for std_dev == 0.0 (:1630); m3 / std_dev.powi(3)
        with the population variance (:1627), times sqrt(n (n - 1)) / (n - 2) (:1638)."""
        st = self._moments(column, L.MOMENTS_WANT_CENTRAL)
        if st["count"] < 3:
            return math.nan
        n = float(st["count"])
        std_dev = _fsqrt(st["m2"] / n)
        if std_dev == 0.0:
            return math.nan
        skewness = _fdiv(st["m3"] / n, (std_dev * std_dev) * std_dev)
        return skewness * (_fsqrt(n * (n - 1.0)) / (n - 2.0))

    def kurtosis(self, column):
        """kurtosis (functions.rs:1642-1665): NaN below 4 valid cells (:1646) and for std_dev == 0.0 (:1655); m4 /
        std_dev.powi(4) - 3.0 (:1660), adjusted as (n - 1) / ((n - 2) (n - 3)) * ((n + 1) k + 6) (:1663)."""
        st = self._moments(column, L.MOMENTS_WANT_CENTRAL)
        if st["count"] < 4:
            return math.nan
        n = float(st["count"])
        std_dev = _fsqrt(st["m2"] / n)
        if std_dev == 0.0:
            return math.nan
        kurt = _fdiv(st["m4"] / n, (std_dev * std_dev) * (std_dev * std_dev)) - 3.0
        return ((n - 1.0) / ((n - 2.0) * (n - 3.0))) * ((n + 1.0) * kurt + 6.0)

    def var_column(self, column, ddof=1):
        """var_column (functions.rs:3571-3584): NaN for count <= ddof (:3575), else sum (v - mean)^2 / (n - ddof) (:3581)."""
        ddof = int(ddof)
        if ddof < 0:
            raise InvalidValue("ddof must not be negative, got %d" % ddof)
        st = self._moments(column, L.MOMENTS_WANT_CENTRAL)
        if st["count"] <= ddof:
            return math.nan
        return st["m2"] / (float(st["count"]) - float(ddof))

    def std_column(self, column, ddof=1):
        """std_column (functions.rs:3586-3588): var_column(column, ddof).sqrt()."""
        return _fsqrt(self.var_column(column, ddof))

    def sem(self, column, ddof=1):
        """sem (aggregations.rs:8-23): NaN for count <= ddof (:12); sqrt(sum (v - mean)^2 / (count - ddof)) / sqrt(n) (:18-22)."""
        ddof = int(ddof)
        if ddof < 0:
            raise InvalidValue("ddof must not be negative, got %d" % ddof)
        st = self._moments(column, L.MOMENTS_WANT_CENTRAL)
        if st["count"] <= ddof:
            return math.nan
        variance = st["m2"] / float(st["count"] - ddof)
        return _fsqrt(variance) / math.sqrt(float(st["count"]))

    def mad(self, column):
        """mad (aggregations.rs:26-39): the mean absolute deviation sum |v - mean| / count (:35-36); NaN without a valid cell (:30)."""
        st = self._moments(column, L.MOMENTS_WANT_CENTRAL)
        if st["count"] == 0:
            return math.nan
        return st["abs_dev"] / float(st["count"])

    def prod(self, column):
        """prod (aggregations.rs:42-51): the product of the valid cells; NaN without one (:46).  A range excursion of finite
        cells is not sticky here (pandrs_hip.h, pandrs_hip_moments)."""
        st = self._moments(column, L.MOMENTS_WANT_PROD)
        return st["prod"] if st["count"] else math.nan

    def range(self, column):
        """range (functions.rs:4207-4219): max - min over the valid cells; NaN without one (:4211)."""
        st = self._moments(column, 0)
        return st["max"] - st["min"] if st["count"] else math.nan

    def abs_sum(self, column):
        """abs_sum (functions.rs:4221-4224): sum |v| over the valid cells."""
        return self._moments(column, 0)["abs_sum"]

    def cv(self, column):
        """cv (aggregations.rs:162-181): NaN without a valid cell (:166) and for mean.abs() < EPSILON (:173); sqrt(sum (v -
        mean)^2 / (n - 1.0).max(1.0)) / mean.abs() (:177-180)."""
        st = self._moments(column, L.MOMENTS_WANT_CENTRAL)
        if st["count"] == 0:
            return math.nan
        n, mean = float(st["count"]), st["mean"]
        if abs(mean) < _F64_EPSILON:
            return math.nan
        return _fdiv(_fsqrt(st["m2"] / max(n - 1.0, 1.0)), abs(mean))

    def geometric_mean(self, column):
        """geometric_mean (aggregations.rs:108-122): exp(sum ln v / count) over the cells > 0 (:110-114); NaN without one."""
        st = self._moments(column, L.MOMENTS_WANT_LOG)
        if st["count_pos"] == 0:
            return math.nan
        return _fexp(st["log_sum"] / float(st["count_pos"]))

    def harmonic_mean(self, column):
        """harmonic_mean (aggregations.rs:125-139): count / sum (1.0 / v) over the cells != 0.0 (:127-131); NaN without one."""
        st = self._moments(column, L.MOMENTS_WANT_RECIP)
        if st["count_nonzero"] == 0:
            return math.nan
        return _fdiv(float(st["count_nonzero"]), st["recip_sum"])

    def iqr(self, column):
        """iqr (aggregations.rs:142-159): sorted[(n * 0.75) as usize] - sorted[(n * 0.25) as usize]; NaN below 2 valid cells (:146)."""
        (q25, q75), m = self._order_stats(column, [(L.OS_AT_FRAC_N, 0.25), (L.OS_AT_FRAC_N, 0.75)])
        return math.nan if m < 2 else float(q75) - float(q25)

    def percentile_value(self, column, q):
        """percentile_value (aggregations.rs:184-200): sorted[((n - 1) * q) as usize]; NaN for q outside [0, 1] (:185), decided
        before any device call, and without a valid cell (:192).  Deviations: the column is looked up first, so a missing or
        non-numeric column raises ColumnNotFound / ColumnTypeMismatch even for a q outside [0, 1] (the reference returns NaN
        there before it looks at the column); a NaN q raises InvalidValue (the reference's comparisons let it through and
        `NaN as usize` indexes element 0)."""
        self._numeric(column)
        q = float(q)
        if math.isnan(q):
            raise InvalidValue("q must not be NaN")
        if q < 0.0 or q > 1.0:
            return math.nan
        (v,), _ = self._order_stats(column, [(L.OS_AT_FRAC_N1, q)])
        return float(v)

    def trimmed_mean(self, column, trim_fraction):
        """trimmed_mean (aggregations.rs:203-225): the mean of sorted[t .. n - t), t = (n * trim_fraction) as usize; NaN for a
        fraction outside [0, 0.5) (:204), decided before any device call, without a valid cell (:211) and for an empty slice
        (:220).  Deviations: the column is looked up first, so a missing or non-numeric column raises ColumnNotFound /
        ColumnTypeMismatch even for a fraction outside [0, 0.5) (the reference returns NaN there before it looks at the
        column); a NaN fraction raises InvalidValue (the reference's comparisons let it through and `NaN as usize` trims
        nothing)."""
        self._numeric(column)
        a = float(trim_fraction)
        if math.isnan(a):
            raise InvalidValue("trim_fraction must not be NaN")
        if a < 0.0 or a >= 0.5:
            return math.nan
        (v,), _ = self._order_stats(column, [(L.OS_TRIMMED_MEAN, a)])
        return float(v)

    def describe_column(self, column):
        """describe_column (aggregations.rs:54-105): {count, mean, std (n - 1, at least 1), min, max, 25%, 50%, 75%} with the
        quartiles sorted[(n * 0.25) as usize], sorted[n / 2], sorted[(n * 0.75) as usize] (:87-89); without a valid cell only
        count 0.0 and NaN mean / std / min / max (:60-67).  One moments call plus one order-statistics call."""
        st = self._moments(column, L.MOMENTS_WANT_CENTRAL)
        if st["count"] == 0:
            return {"count": 0.0, "mean": math.nan, "std": math.nan, "min": math.nan, "max": math.nan}
        n = float(st["count"])
        (q25, q50, q75), _ = self._order_stats(column, [(L.OS_AT_FRAC_N, 0.25), (L.OS_AT_FRAC_N, 0.5), (L.OS_AT_FRAC_N, 0.75)])
        # (n * 0.5) as usize == n / 2 for every n below 2^53: halving is exact
        return {"count": n, "mean": st["mean"], "std": _fsqrt(st["m2"] / max(n - 1.0, 1.0)), "min": st["min"], "max": st["max"],
                "25%": float(q25), "50%": float(q50), "75%": float(q75)}

    def zscore(self, column):
        """zscore (functions.rs:2284-2314): (v - mean) / std_dev with the sample deviation (n - 1, :2296), NaN stays NaN, -> list
        of float.  InvalidValue where the reference returns Err: fewer than 2 valid cells (:2288), a deviation of zero (:2298).
        One moments call plus one pandrs_hip_eval call."""
        st = self._moments(column, L.MOMENTS_WANT_CENTRAL)
        if st["count"] < 2:
            raise InvalidValue("Need at least 2 values for z-score")
        std_dev = _fsqrt(st["m2"] / (float(st["count"]) - 1.0))
        if std_dev == 0.0:
            raise InvalidValue("Standard deviation is zero")
        out = self._eval_values((col(column) - st["mean"]) / std_dev)
        values = np.array(out.data, dtype=np.float64)
        if out.null_mask is not None:                      # a null cell is the mirrors' missing value: NaN, as a NaN cell
            values[np.unpackbits(np.asarray(out.null_mask, np.uint8), bitorder="little")[:values.shape[0]].astype(bool)] = np.nan
        return values.tolist()

    def _moments_all(self, want):
        """[(name, stats)] of every Int64 / Float64 column in column order (the reference's `if let Ok(values) =
        get_column_numeric_values`): all of them in one call per L.MOMENTS_MAX_COLUMNS columns."""
        names = [n for n in self.column_names if self.column(n).dtype in (L.I64, L.F64)]
        out = []
        for i in range(0, len(names), L.MOMENTS_MAX_COLUMNS):
            chunk = names[i:i + L.MOMENTS_MAX_COLUMNS]
            stats = get_context().moments([self.column(n).view() for n in chunk], self._row_count, want)
            out.extend(zip(chunk, stats))
        return out

    def sum_all(self):
        """sum_all (functions.rs:934-943): [(name, sum of the valid cells)] of every numeric column."""
        return [(n, st["sum"]) for n, st in self._moments_all(0)]

    def mean_all(self):
        """mean_all (functions.rs:944-957): sum / count; a column without a valid cell is left out (:950)."""
        return [(n, st["mean"]) for n, st in self._moments_all(0) if st["count"]]

    def var_all(self):
        """var_all (functions.rs:975-991): sum (v - mean)^2 / (count - 1); a column with fewer than 2 valid cells is left out (:981)."""
        return [(n, st["m2"] / float(st["count"] - 1)) for n, st in self._moments_all(L.MOMENTS_WANT_CENTRAL) if st["count"] > 1]

    def std_all(self):
        """std_all (functions.rs:958-974): var_all's values, square-rooted (:969)."""
        return [(n, _fsqrt(v)) for n, v in self.var_all()]

    def min_all(self):
        """min_all (functions.rs:992-1005): the fold of f64::min from +inf; a column without a valid cell is left out (:998)."""
        return [(n, st["min"]) for n, st in self._moments_all(0) if st["count"]]

    def max_all(self):
        """max_all (functions.rs:1006-1022): the fold of f64::max from -inf; a column without a valid cell is left out (:1012)."""
        return [(n, st["max"]) for n, st in self._moments_all(0) if st["count"]]

    def product_all(self):
        """product_all (functions.rs:1583-1595): the product from 1.0; a column without a valid cell is left out (:1588)."""
        return [(n, st["prod"]) for n, st in self._moments_all(L.MOMENTS_WANT_PROD) if st["count"]]

    def median_all(self):
        """median_all (functions.rs:1597-1615): (sorted[n/2 - 1] + sorted[n/2]) / 2.0 for even n, else sorted[n/2] (:1604-1609);
        a column without a valid cell is left out (:1602).  One order-statistics call per numeric column."""
        out = []
        for n in self.column_names:
            c = self.column(n)
            if c.dtype in (L.I64, L.F64):
                (v,), m = get_context().order_stats(c.view(), c.len(), [(L.OS_MEDIAN, 0.0)])
                if m:
                    out.append((n, float(v)))
        return out

    # -- value_range / cut / qcut (dataframe/pandas_compat/functions.rs:2270-2282, :2339-2420) ----------------------
    def value_range(self, column):
        """PandasCompatExt::value_range (functions.rs:2270-2282): (min, max) over the cells that are not NaN, from the
        whole-column reduction.  InvalidValue when there is no such cell.  Errors before any device call: ColumnNotFound,
        ColumnTypeMismatch for a String or Boolean column."""
        c = self._numeric(column)
        if c.len() == 0:
            raise InvalidValue("No valid values in column")
        st = get_context().column_stats(c.view(), c.len())
        lo, hi = float(st["min"]), float(st["max"])
        if lo > hi:                                                      # the fold identities: no cell that is not NaN
            raise InvalidValue("No valid values in column")
        return lo, hi

    def bin_codes(self, column, edges):
        """The bin of every row against a caller's edge list, for callers that go on with the codes (group_by the bucket):
        one pandrs_hip_bin call -> (codes, counts).  codes: int32 numpy array, i where edges[i] <= v < edges[i + 1] (the
        reference's first match), L.BIN_NONE (-1) for a row in no bin, L.BIN_NAN (-2) for a NaN or null cell; counts: int64
        numpy array of len(edges) + 1, the rows per bin, then NONE, then NAN.  `edges` never decrease and hold no NaN
        (InvalidValue otherwise, as for fewer than 2 or more than L.BIN_MAX_BINS + 1 edges)."""
        c = self._numeric(column)
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        if not 2 <= e.shape[0] <= L.BIN_MAX_BINS + 1:
            raise InvalidValue("bin_codes takes 2 to %d edges, got %d" % (L.BIN_MAX_BINS + 1, e.shape[0]))
        if np.isnan(e).any() or (np.diff(e) < 0).any():
            raise InvalidValue("the edges must not decrease and none may be NaN")
        if c.len() == 0:
            return np.empty(0, np.int32), np.zeros(e.shape[0] + 1, np.int64)
        codes, counts = get_context().bin(c.view(), c.len(), e, out_device=False)
        return np.asarray(codes), counts

    def _bin_labels(self, c, kind, k, what):
        """-> (codes or None, edges, NaN rows): the edge list from one pandrs_hip_bin_edges call and the codes from one
        pandrs_hip_bin call against it.  codes is None where the reference's w is not finite: e[0] is NaN then, every bin is
        empty and the result is one "NaN" per NaN row (pandrs_hip.h)."""
        if k > L.BIN_MAX_BINS:
            raise InvalidValue("%s takes at most %d, got %d" % (what, L.BIN_MAX_BINS, k))
        n = c.len()
        ctx = get_context() if n else None
        edges, valid = ctx.bin_edges(c.view(), n, kind, k) if n else (None, 0)
        if valid == 0:
            raise InvalidValue("No valid values in column" if kind == L.BIN_CUT else "No valid values")
        if np.isnan(edges[0]):
            return None, edges, n - valid
        look = edges.copy()
        if kind == L.BIN_QCUT:
            look[k] = edges[k] + 0.001                                   # functions.rs:2406-2407
        elif look[k] < look[k - 1]:
            look[k] = look[k - 1]                                        # (for the search only: no row lies between them)
        codes, _ = ctx.bin(c.view(), n, look, out_device=False, want_counts=False)
        return np.asarray(codes), edges, n - valid

    def cut(self, column, bins):
        """PandasCompatExt::cut (functions.rs:2339-2368): `bins` equal-width bins over [min, max] of the cells that are not
        NaN, the last edge max + 0.001; -> the reference's Vec<String>: "(lo, hi]" with two decimals for the first bin with
        lo <= v < hi, "NaN" for a NaN or null cell, and NO entry for a row that matches no bin (the maximum once max + 0.001
        == max, from about 2^43 upward): the list is then shorter than the column, as the reference's is.  One
        pandrs_hip_bin_edges and one pandrs_hip_bin call; at most `bins` labels are formatted.  InvalidValue for bins == 0 or
        no valid cell; ColumnNotFound / ColumnTypeMismatch before any device call.  Deviation (pandrs_hip.h): an edge that
        is zero may read "-0.00"."""
        c = self._numeric(column)
        bins = int(bins)
        if bins <= 0:
            raise InvalidValue("Number of bins must be > 0")
        codes, edges, n_nan = self._bin_labels(c, L.BIN_CUT, bins, "cut: bins")
        if codes is None:
            return ["NaN"] * n_nan
        labels = np.empty(bins + 2, dtype=object)                        # code -> label, "NaN" behind the bins; NONE has none
        for i in np.unique(codes[codes >= 0]):                           # (only the bins that hold a row are formatted)
            labels[i] = "(%.2f, %.2f]" % (edges[i], edges[i + 1])
        labels[bins + 1] = "NaN"
        kept = codes[codes != L.BIN_NONE]
        return labels[np.where(kept == L.BIN_NAN, bins + 1, kept)].tolist()

    def qcut(self, column, q):
        """PandasCompatExt::qcut (functions.rs:2370-2420): edges at the order statistics valid[min(m * i / q, m - 1)] of the
        m cells that are not NaN, the last one + 0.001 for the look-up; -> the reference's Vec<String>: "Q{i + 1}" for the
        first i with e[i] <= v < e[i + 1], "NaN" for a NaN or null cell, "" for a row that matches no bin.  One
        pandrs_hip_bin_edges call (the radix select of describe, no sort) and one pandrs_hip_bin call.  InvalidValue for
        q == 0 or no valid cell; ColumnNotFound / ColumnTypeMismatch before any device call."""
        c = self._numeric(column)
        q = int(q)
        if q <= 0:
            raise InvalidValue("Number of quantiles must be > 0")
        codes, _, _ = self._bin_labels(c, L.BIN_QCUT, q, "qcut: q")
        labels = np.array(["Q%d" % (i + 1) for i in range(q)] + ["", "NaN"], dtype=object)
        return labels[np.where(codes >= 0, codes, q - 1 - codes)].tolist()

    # -- value_counts / unique / nunique / mode / is_unique (dataframe/pandas_compat/functions.rs:343-384, :775-788, -------
    #    :1709-1753, :4120-4139, :4226-4259): one pandrs_hip_distinct call each, the list of distinct values on the host ----
    def _distinct(self, col, order):
        """-> (values, flags, counts, info) of one pandrs_hip_distinct call; a String column orders by its strings (the pool's
        rank table).  No rows: an empty list, no device call."""
        n = col.len()
        if n == 0:
            return (np.empty(0, np.uint64), np.empty(0, np.uint8), np.empty(0, np.int64),
                    {"n_entries": 0, "n_valid": 0, "nan_count": 0, "null_count": 0, "max_count": 0, "n_modes": 0, "path": 0})
        rank = GLOBAL_STRING_POOL.rank_table() if col.dtype == L.U32CODE else None
        v, f, k, info = get_context().distinct(col.view(), n, order, code_rank=rank, out_device=False)
        return np.asarray(v, np.uint64), np.asarray(f, np.uint8), np.asarray(k, np.int64), info

    @staticmethod
    def _cells_as_f64(col, values):
        """Entry cells of a numeric column as the reference's f64 values (an Int64 cell `as f64`)."""
        if col.dtype == L.F64:
            return values.view(np.float64)
        return values.view(np.int64).astype(np.float64)

    def _string_entries(self, col, order):
        """-> [(string, count)] in the device's order: the strings get_column_string_values gives for the column (an Int64 /
        Float64 cell's to_string, "true" / "false"), a missing cell as "NaN" for a numeric column and as "" otherwise - merged
        with the "" / "NaN" the column may hold itself.  `merged` says whether an entry's count changed on the host."""
        v, f, k, _ = self._distinct(col, order)
        number = f == L.DISTINCT_NUMBER
        strings = _key_strings(col.dtype, v[number], np.zeros(int(number.sum()), np.uint8))
        entries = list(zip(strings, k[number].tolist()))
        missing = int(k[~number].sum())
        if not missing:
            return entries, False
        name = "NaN" if col.dtype in (L.I64, L.F64) else ""
        for i, (s, c) in enumerate(entries):
            if s == name:
                entries[i] = (s, c + missing)
                return entries, True
        entries.append((name, missing))
        return entries, True

    def _string_typed(self, column):
        col = self.column(column)
        if col.dtype != L.U32CODE:
            raise ColumnTypeMismatch(L.ERR_TYPE_MISMATCH, "Column '%s' is not a string type" % column)
        return col

    def value_counts(self, column):
        """PandasCompatExt::value_counts (functions.rs:359-368): [(string, count)], count descending, ties by string (byte-wise)
        - for a String column the device's own order (pandrs_hip_distinct BY_COUNT through the pool's rank table); any other
        column is counted by value and its entries ordered by their strings on the host, as the reference stringifies first.
        A missing cell counts as "" (String, Boolean) or "NaN" (numeric).  ColumnNotFound before any device call."""
        col = self.column(column)
        entries, merged = self._string_entries(col, L.DISTINCT_BY_COUNT)
        if merged or col.dtype != L.U32CODE:
            entries.sort(key=lambda e: (-e[1], e[0].encode()))
        return entries

    def value_counts_numeric(self, column):
        """PandasCompatExt::value_counts_numeric (functions.rs:369-384): [(f64, count)], count descending, ties by value.  One
        (NaN, nan_count + null_count) entry for the NaN and null cells together, after the numbers of its count.  Deviations
        (pandrs_hip.h): every NaN payload is one entry; -0.0 comes before 0.0 among equal counts (the reference: HashMap
        order); Int64 cells are counted as integers (beyond 2^53 two entries may print as the same float).  ColumnNotFound /
        ColumnTypeMismatch before any device call."""
        col = self._numeric(column)
        v, f, k, info = self._distinct(col, L.DISTINCT_BY_COUNT)
        number = f == L.DISTINCT_NUMBER
        out = list(zip(self._cells_as_f64(col, v[number]).tolist(), k[number].tolist()))
        missing = info["nan_count"] + info["null_count"]
        if missing:
            at = int(np.searchsorted(-k[number], -missing, side="right"))
            out.insert(at, (math.nan, missing))
        return out

    def unique(self, column):
        """PandasCompatExt::unique (functions.rs:775-781): the column's distinct strings, ascending byte-wise."""
        col = self.column(column)
        entries, _ = self._string_entries(col, L.DISTINCT_BY_VALUE)
        return sorted((s for s, _ in entries), key=str.encode)         # (a String column arrives in this order already)

    def unique_numeric(self, column):
        """PandasCompatExt::unique_numeric (functions.rs:782-788): the distinct values ascending, -0.0 before 0.0, one NaN last
        when a cell is NaN or null (the reference: every payload, wherever its sort leaves them)."""
        col = self._numeric(column)
        v, f, _, info = self._distinct(col, L.DISTINCT_BY_VALUE)
        out = self._cells_as_f64(col, v[f == L.DISTINCT_NUMBER]).tolist()
        return out + ([math.nan] if info["nan_count"] + info["null_count"] else [])

    def nunique(self):
        """PandasCompatExt::nunique (functions.rs:343-352): [(column, number of distinct strings)] for every column, a missing
        cell as in value_counts."""
        return [(name, len(self._string_entries(self.column(name), L.DISTINCT_BY_VALUE)[0])) for name in self.column_names]

    def nunique_all(self):
        """PandasCompatExt::nunique_all (functions.rs:4120-4139): {column: distinct values}; NaN and missing cells are left out."""
        out = {}
        for name in self.column_names:
            info = self._distinct(self.column(name), L.DISTINCT_BY_VALUE)[3]
            out[name] = info["n_entries"] - (1 if info["nan_count"] else 0) - (1 if info["null_count"] else 0)
        return out

    def mode_numeric(self, column):
        """PandasCompatExt::mode_numeric (functions.rs:1709-1730): the numbers with the largest count, ascending; [] when the
        column holds no number."""
        col = self._numeric(column)
        v, f, k, info = self._distinct(col, L.DISTINCT_BY_VALUE)
        keep = (f == L.DISTINCT_NUMBER) & (k == info["max_count"])
        return self._cells_as_f64(col, v[keep]).tolist() if info["max_count"] else []

    def mode_string(self, column):
        """PandasCompatExt::mode_string (functions.rs:1732-1753): the strings with the largest count, ascending; the "" entry
        (and with it every missing cell) is dropped first."""
        col = self._string_typed(column)
        entries = [(s, c) for s, c in self._string_entries(col, L.DISTINCT_BY_VALUE)[0] if s != ""]
        if not entries:
            return []
        top = max(c for _, c in entries)
        return sorted((s for s, c in entries if c == top), key=str.encode)

    def mode_with_count(self, column):
        """PandasCompatExt::mode_with_count (functions.rs:4243-4259): (the most frequent number, its count); (NaN, 0) when
        there is no number.  Among numbers of the same count this returns the SMALLEST (the reference: whichever its HashMap
        iterates last)."""
        col = self._numeric(column)
        v, f, k, info = self._distinct(col, L.DISTINCT_BY_COUNT)
        number = np.flatnonzero(f == L.DISTINCT_NUMBER)
        if number.size == 0:
            return (math.nan, 0)
        first = number[:1]                                               # BY_COUNT: the largest count, then the smallest value
        return (float(self._cells_as_f64(col, v[first])[0]), int(k[first][0]))

    def is_unique(self, column):
        """PandasCompatExt::is_unique (functions.rs:4226-4241): no value occurs twice among the cells that are neither NaN nor
        missing."""
        info = self._distinct(self.column(column), L.DISTINCT_BY_VALUE)[3]
        numbers = info["n_entries"] - (1 if info["nan_count"] else 0) - (1 if info["null_count"] else 0)
        return numbers == info["n_valid"]

    # -- crosstab / pivot_table / pivot / unstack (dataframe/pandas_compat/functions.rs:2138-2183, :2471-2527, ------------
    #    pivot/mod.rs:12-250): one pandrs_hip_pivot call each, the small label x label matrix ordered on the host -----------
    def _pivot_labels(self, col, cells, flags, counts_add, what):
        """The strings of one dimension's labels and the order the reference gives them.  -> (strings, take): `take` lists, per
        output label in byte-wise ascending order, the device labels that form it.  A label is stringified as value_counts does
        (an Int64 / Float64 cell's to_string, the pooled string, "true" / "false"); the missing label is "NaN" for a numeric
        column and "" otherwise.  A missing label that reads like a literal label of the same String / Boolean column is the
        same string to the reference: the two are merged where counts add (crosstab), and an OperationFailed otherwise."""
        number = flags == L.PIVOT_NUMBER
        strings = _key_strings(col.dtype, cells[number], np.zeros(int(number.sum()), np.uint8))
        if not number.all():
            strings.append("NaN" if col.dtype in (L.I64, L.F64) else "")
        groups = {}
        for i, s in enumerate(strings):
            groups.setdefault(s, []).append(i)
        if len(groups) != len(strings) and not counts_add:
            raise OperationFailed(L.ERR_OPERATION_FAILED, "%s: a missing cell of the key column reads like its label %r; the two "
                                  "cannot share a cell" % (what, "NaN" if col.dtype in (L.I64, L.F64) else ""))
        names = sorted(groups, key=str.encode)
        return names, [groups[s] for s in names]

    def _pivot(self, index, columns, values, op, what):
        """-> (index column, index strings, column strings, cells (C, R) float64, rows (C, R) int64) of one pandrs_hip_pivot
        call, rows and columns in byte-wise string order.  ColumnNotFound and type errors come before any device call; a
        columns label equal to the index column's name is DuplicateColumnName."""
        icol, ccol = self.column(index), self.column(columns)
        vcol = None
        if values is not None:
            if values not in self.column_indices:
                raise ColumnNotFound(values)
            vcol = self._numeric(values)
        n = self._row_count
        if n == 0:
            return icol, [], [], np.empty((0, 0), np.float64), np.empty((0, 0), np.int64)
        ranks = [GLOBAL_STRING_POOL.rank_table() if c.dtype == L.U32CODE else None for c in (icol, ccol)]
        il, fi, cl, fc, cells, rows, _ = get_context().pivot(icol.view(), ccol.view(), n, op, None if vcol is None else vcol.view(),
                                                             index_rank=ranks[0], columns_rank=ranks[1], out_device=False)
        add = op == L.PIVOT_ROWS
        inames, itake = self._pivot_labels(icol, np.asarray(il, np.uint64), np.asarray(fi, np.uint8), add, what)
        cnames, ctake = self._pivot_labels(ccol, np.asarray(cl, np.uint64), np.asarray(fc, np.uint8), add, what)
        if index in cnames:
            raise DuplicateColumnName(index)
        cells, rows = np.asarray(cells, np.float64), np.asarray(rows, np.int64)
        if add:                                                 # merged labels: their rows add
            rows = np.stack([rows[t].sum(axis=0) for t in ctake]) if ctake else rows
            rows = np.stack([rows[:, t].sum(axis=1) for t in itake], axis=1) if itake else rows
            cells = rows.astype(np.float64)
        else:
            cells = cells[[t[0] for t in ctake]][:, [t[0] for t in itake]]
            rows = rows[[t[0] for t in ctake]][:, [t[0] for t in itake]]
        return icol, inames, cnames, cells, rows

    def crosstab(self, col1, col2):
        """PandasCompatExt::crosstab (functions.rs:2138-2183): a String column `col1` with the distinct strings of col1 ascending
        byte-wise, and one Float64 column per distinct string of col2, ascending, holding the number of rows with that pair
        (0.0 where there is none).  A missing cell reads "" (String, Boolean) or "NaN" (numeric), as in value_counts."""
        _, inames, cnames, cells, _ = self._pivot(col1, col2, None, L.PIVOT_ROWS, "crosstab")
        out = OptimizedDataFrame()
        out.add_column(col1, StringColumn(inames))
        for j, name in enumerate(cnames):
            out.add_column(name, Float64Column(cells[j]))
        return out

    def pivot_table(self, index, columns, values, aggfunc):
        """DataFrame::pivot_table (pivot/mod.rs:107-250): a String column `index` with the distinct index strings and one Float64
        column per distinct columns string holding Sum / Mean / Min / Max / Count of `values` over the rows of the pair, with the
        engine's fold rules (pandrs_hip.h).  Deviations: the reference's legacy frame writes every cell as a string, "" for a
        pair without rows - here Float64 columns with a null mask on those cells (the value under it NaN); its label order is
        HashSet order - here byte-wise ascending, as in crosstab."""
        if not isinstance(aggfunc, AggFunction):
            got = AggFunction.from_str(aggfunc)
            if got is None:
                raise InvalidValue("unknown aggregation function %r" % (aggfunc,))
            aggfunc = got
        op = {AggFunction.Sum: L.PIVOT_SUM, AggFunction.Mean: L.PIVOT_MEAN, AggFunction.Min: L.PIVOT_MIN, AggFunction.Max: L.PIVOT_MAX,
              AggFunction.Count: L.PIVOT_COUNT}[aggfunc]
        _, inames, cnames, cells, rows = self._pivot(index, columns, values, op, "pivot_table")
        out = OptimizedDataFrame()
        out.add_column(index, StringColumn(inames))
        for j, name in enumerate(cnames):
            out.add_column(name, Float64Column.with_nulls(cells[j], rows[j] == 0))
        return out

    def unstack(self, index_col, columns_col, values_col):
        """PandasCompatExt::unstack (functions.rs:2471-2522): as crosstab's shape, every cell the value of the LAST row holding the
        pair (the reference inserts into a HashMap row by row), NaN where no row holds it, no null mask; a null value cell
        reads 0.0."""
        _, inames, cnames, cells, _ = self._pivot(index_col, columns_col, values_col, L.PIVOT_LAST, "unstack")
        out = OptimizedDataFrame()
        out.add_column(index_col, StringColumn(inames))
        for j, name in enumerate(cnames):
            out.add_column(name, Float64Column(cells[j]))
        return out

    def pivot(self, index, columns, values):
        """PandasCompatExt::pivot (functions.rs:2524-2527): unstack."""
        return self.unstack(index, columns, values)

    # -- cumulative folds and lags (dataframe/pandas_compat/functions.rs:280-342, :514-541, :2081-2094) ------------
    def _cumulative(self, column_name, op):
        """One pandrs_hip_cumulative call -> the values as a host array.  Errors before any device call: ColumnNotFound,
        ColumnTypeMismatch for a String or Boolean column (as rank); an empty column gives an empty result."""
        col = self._numeric(column_name)
        if col.len() == 0:
            return np.empty(0, np.int64 if op == L.CUM_COUNT else np.float64)
        return np.asarray(get_context().cumulative(col.view(), col.len(), op, out_device=False)[0])

    def _lag(self, column_name, op, periods):
        col = self._numeric(column_name)
        periods = int(periods)
        if op != L.LAG_SHIFT and periods < 0:
            raise InvalidValue("periods must not be negative, got %d" % periods)        # the reference takes a usize
        if col.len() == 0:
            return np.empty(0, np.float64), None
        values, mask, _ = get_context().lag(col.view(), col.len(), op, periods, out_device=False)
        return np.asarray(values), mask

    def cumsum(self, column):
        """PandasCompatExt::cumsum (functions.rs:280-291): the running sum from +0.0, -> list of float.  A NaN cell makes
        every later row NaN.  Deviation (pandrs_hip.h): a row under a null bit is skipped and answers NaN; the parallel sum
        is within 2 gamma_k sum|x| of the sequential one, and bit for bit on integer-valued data below 2^53."""
        return self._cumulative(column, L.CUM_SUM).tolist()

    def cumprod(self, column):
        """PandasCompatExt::cumprod (functions.rs:292-303): the running product from 1.0, -> list of float; sticky after an
        overflow or an underflow to zero, as the reference's fold."""
        return self._cumulative(column, L.CUM_PROD).tolist()

    def cummax(self, column):
        """PandasCompatExt::cummax (functions.rs:304-315): the f64::max fold from -inf, NaN cells skipped, -> list of float."""
        return self._cumulative(column, L.CUM_MAX).tolist()

    def cummin(self, column):
        """PandasCompatExt::cummin (functions.rs:316-327): the f64::min fold from +inf, NaN cells skipped, -> list of float."""
        return self._cumulative(column, L.CUM_MIN).tolist()

    def cumcount(self, column):
        """PandasCompatExt::cumcount (functions.rs:2081-2094): the rows so far that are neither NaN nor null, -> list of int."""
        return [int(v) for v in self._cumulative(column, L.CUM_COUNT)]

    def shift(self, column, periods):
        """PandasCompatExt::shift (functions.rs:328-342): row i takes the cell of row i - periods, -> list of float or None
        (no source row, or a null one)."""
        values, mask = self._lag(column, L.LAG_SHIFT, periods)
        out = values.tolist()
        if mask is not None:
            for i in np.flatnonzero(np.unpackbits(mask, bitorder="little")[:len(out)]):
                out[i] = None
        return out

    def diff(self, column, periods):
        """PandasCompatExt::diff (functions.rs:531-541): x[i] - x[i - periods], NaN for rows i < periods, -> list of float."""
        return self._lag(column, L.LAG_DIFF, periods)[0].tolist()

    def pct_change(self, column, periods):
        """PandasCompatExt::pct_change (functions.rs:514-530): (x[i] - prev) / prev with prev = x[i - periods]; NaN for rows
        i < periods and where prev == 0.0, -> list of float."""
        return self._lag(column, L.LAG_PCT_CHANGE, periods)[0].tolist()

    # -- missing values (dataframe/pandas_compat/functions.rs:789-918, :3626-3683) ------------------------------
    def _fill(self, column_name, method, value=None):
        """One pandrs_hip_fill call -> a NEW frame: the named column replaced (same name, same position; Float64 after
        interpolate; a null mask only when rows are still missing), the other columns shared unchanged.  A cell is
        missing when its null bit is set or, for Float64, when it is NaN.  Errors before any device call:
        ColumnNotFound, ColumnTypeMismatch for a String or Boolean column (as describe and rank).  Deviations
        (pandrs_hip.h): the reference casts every numeric column to f64 and knows no null mask here; Int64 stays Int64
        under ffill / bfill / fillna."""
        col = self.column(column_name)
        if col.dtype not in (L.I64, L.F64):
            raise ColumnTypeMismatch(L.ERR_TYPE_MISMATCH, "Column '%s' is not a numeric type" % column_name)
        if col.len() == 0:
            new = col
        else:
            values, mask, _ = get_context().fill(col.view(), col.len(), method, value, out_device=False)
            new = (Int64Column if values.dtype == np.int64 else Float64Column)(values)
            new.null_mask = mask
        result = OptimizedDataFrame()
        for name in self.column_names:
            result.add_column(name, new if name == column_name else self.column(name))
        return result

    def ffill(self, column_name):
        """ffill (functions.rs:3626-3653): every missing row takes the cell of the last valid row before it; rows in
        front of the first valid row stay missing."""
        return self._fill(column_name, L.FILL_FFILL)

    def bfill(self, column_name):
        """bfill (functions.rs:3655-3683): every missing row takes the cell of the next valid row after it; rows behind
        the last valid row stay missing."""
        return self._fill(column_name, L.FILL_BFILL)

    def fillna_method(self, column_name, method):
        """fillna_method (functions.rs:811-868): "ffill" | "forward" | "bfill" | "backward"."""
        self.column(column_name)
        if method in ("ffill", "forward"):
            return self.ffill(column_name)
        if method in ("bfill", "backward"):
            return self.bfill(column_name)
        raise InvalidValue("Invalid fill method: '%s'. Use 'ffill' or 'bfill'." % (method,))        # functions.rs:846-851

    def interpolate(self, column_name):
        """interpolate (functions.rs:870-918): a missing row between the valid rows p < i < q becomes
        a + ((b - a) * (i - p)) / (q - p); rows outside the first and last valid row stay missing.  Float64 always."""
        return self._fill(column_name, L.FILL_LINEAR)

    def fillna(self, column_name, value):
        """fillna (functions.rs:789-809): every missing row becomes `value` (an int for an Int64 column, a float for
        Float64; NaN leaves the rows missing, as in the reference)."""
        return self._fill(column_name, L.FILL_VALUE, value)

    # -- row masks (dataframe/pandas_compat/helpers/comparison_ops.rs:7-46, functions.rs:141-158, :253-257, :4141-4161) ----
    def _predicate(self, column_name, op, a=0.0, b=0.0):
        """One pandrs_hip_predicate call -> the reference's Vec<bool> as a list of bool.  Every compare happens in f64 (an
        Int64 cell as `v as f64`); a cell under a null bit behaves as NaN (pandrs_hip.h: the reference fails on a missing
        value).  Errors before any device call: ColumnNotFound, ColumnTypeMismatch for a String or Boolean column."""
        col = self._numeric(column_name)
        if col.len() == 0:
            return []
        bits, _ = get_context().predicate(col.view(), col.len(), op, a, b, out_device=False)
        return np.unpackbits(bits, count=col.len(), bitorder="little").astype(bool).tolist()

    def _predicate_count(self, column_name, op, a=0.0):
        col = self._numeric(column_name)
        if col.len() == 0:
            return 0
        return get_context().predicate(col.view(), col.len(), op, a, count_only=True)[1]

    def _predicate_rows(self, column_name, op, a=0.0):
        """predicate -> filter_indices on the device mask -> filter_gather per column: the mask does not visit the host.
        The result is filter's (nulls become 0 / 0.0 / "" / false, no masks; no selected row: every column with 0 rows)."""
        col = self._numeric(column_name)
        if self._row_count == 0:
            return self._empty_columns()
        bits, _ = get_context().predicate(col.view(), self._row_count, op, a, out_device=True)
        return self._compact((bits, None, L.BOOLBITS))[0]

    def gt(self, column, value):
        """gt (comparison_ops.rs:7-10): !v.is_nan() && v > value per row."""
        return self._predicate(column, L.PRED_GT, value)

    def ge(self, column, value):
        """ge (comparison_ops.rs:13-16)."""
        return self._predicate(column, L.PRED_GE, value)

    def lt(self, column, value):
        """lt (comparison_ops.rs:19-22)."""
        return self._predicate(column, L.PRED_LT, value)

    def le(self, column, value):
        """le (comparison_ops.rs:25-28)."""
        return self._predicate(column, L.PRED_LE, value)

    def eq_value(self, column, value):
        """eq_value (comparison_ops.rs:31-37): !v.is_nan() && (v - value).abs() < f64::EPSILON."""
        return self._predicate(column, L.PRED_EQ, value)

    def ne_value(self, column, value):
        """ne_value (comparison_ops.rs:40-46): v.is_nan() || (v - value).abs() >= f64::EPSILON."""
        return self._predicate(column, L.PRED_NE, value)

    def between(self, column, lower, upper):
        """between (functions.rs:253-257): lower <= v && v <= upper."""
        return self._predicate(column, L.PRED_BETWEEN, lower, upper)

    def is_between(self, column, lower, upper, inclusive=True):
        """is_between (functions.rs:4141-4161): between, or lower < v && v < upper when not inclusive."""
        return self._predicate(column, L.PRED_BETWEEN if inclusive else L.PRED_BETWEEN_EXCLUSIVE, lower, upper)

    def isna(self, column):
        """isna (functions.rs:930-933): v.is_nan(); a null cell counts as NaN here."""
        return self._predicate(column, L.PRED_ISNA)

    def notna(self, column):
        """notna (functions.rs:1312-1315)."""
        return self._predicate(column, L.PRED_NOTNA)

    def is_finite(self, column):
        """is_finite (functions.rs:4016-4019)."""
        return self._predicate(column, L.PRED_IS_FINITE)

    def is_infinite(self, column):
        """is_infinite (functions.rs:4021-4024)."""
        return self._predicate(column, L.PRED_IS_INFINITE)

    def count_na(self, column):
        """count_na (functions.rs:3837-3840): the NaN (and null) cells, from the count-only form: no mask is written."""
        return self._predicate_count(column, L.PRED_ISNA)

    def has_nulls(self, column):
        """has_nulls (functions.rs:4187-4190)."""
        return self._predicate_count(column, L.PRED_ISNA) > 0

    def count_value(self, column, value):
        """count_value (functions.rs:4089-4095): the cells eq_value selects, counted on the device."""
        return self._predicate_count(column, L.PRED_EQ, value)

    def query_gt(self, column, value):
        """query_gt (functions.rs:2785-2789): the rows with v > value, every column kept, assembled as filter does."""
        return self._predicate_rows(column, L.PRED_GT, value)

    def query_lt(self, column, value):
        """query_lt (functions.rs:2791-2795)."""
        return self._predicate_rows(column, L.PRED_LT, value)

    def query_eq(self, column, value):
        """query_eq (functions.rs:2776-2783): the rows with (v - value).abs() < f64::EPSILON."""
        return self._predicate_rows(column, L.PRED_EQ, value)

    def dropna(self, column):
        """dropna (functions.rs:920-929): the rows whose cell is not NaN (and not null), every column kept."""
        return self._predicate_rows(column, L.PRED_NOTNA)

    def isin_numeric(self, column, values):
        """isin_numeric (functions.rs:150-158): the cell's f64 bits are in the list's (-0.0 is not 0.0; a NaN matches the
        same payload only).  A null cell never matches."""
        col = self._numeric(column)
        vals = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        if col.len() == 0:
            return []
        bits, _ = get_context().isin(col.view(), col.len(), (vals, None, L.F64), out_device=False)
        return np.unpackbits(bits, count=col.len(), bitorder="little").astype(bool).tolist()

    def isin(self, column, values):
        """isin (functions.rs:141-149) on a String column, through pool codes: a string the pool has never seen cannot be
        in the column and is dropped from the list.  A null cell never matches.  Errors before any device call:
        ColumnNotFound, ColumnTypeMismatch for a column that is not String."""
        col = self.column(column)
        if col.dtype != L.U32CODE:
            raise ColumnTypeMismatch(L.ERR_TYPE_MISMATCH, "Column '%s' is not a string type" % column)
        codes = [c for c in map(GLOBAL_STRING_POOL.find, values) if c is not None]
        if col.len() == 0:
            return []
        bits, _ = get_context().isin(col.view(), col.len(), (np.asarray(codes, dtype=np.uint32), None, L.U32CODE), out_device=False)
        return np.unpackbits(bits, count=col.len(), bitorder="little").astype(bool).tolist()

    # -- derived columns (dataframe/pandas_compat/functions.rs:237, :1079-1139, :2316, :2819-2960, :3846-4110; helpers/math_ops.rs) --
    def _bind(self, expr):
        """An expression -> (column views, postfix program, is_mask), checked on the host before any device call:
        ColumnNotFound, ColumnTypeMismatch for a String column (the message rank and describe use), InvalidValue for a type
        or limit error of the program (pandrs_hip_eval_check, which needs no device)."""
        if not isinstance(expr, Expr):
            raise InvalidValue("expected an expression built from col() / lit() / where(), got %r" % (expr,))
        names, program = expr.lower()
        if not names:
            raise InvalidValue("the expression names no column")
        cols = [self.column(name) for name in names]
        for name, c in zip(names, cols):
            if c.dtype not in (L.I64, L.F64, L.BOOLBITS):
                raise ColumnTypeMismatch(L.ERR_TYPE_MISMATCH, "Column '%s' is not a numeric type" % name)
        try:
            is_mask, _ = Context.eval_check([c.dtype for c in cols], program)
        except PandrsHipError as e:
            raise InvalidValue(str(e))
        return [c.view() for c in cols], program, is_mask

    def _eval_values(self, expr):
        """One pandrs_hip_eval call of a value expression -> a Float64Column (a null mask only where rows are null)."""
        views, program, is_mask = self._bind(expr)
        if is_mask:
            raise InvalidValue("the expression is a condition; a column takes a value (use where(cond, a, b))")
        if self._row_count == 0:
            return Float64Column([])
        values, mask, _ = get_context().eval(views, self._row_count, program, out_device=False)
        new = Float64Column(values)
        new.null_mask = mask
        return new

    def _replaced(self, column_name, new):
        """A NEW frame with the named column replaced in position, the others shared, as _fill builds its result."""
        result = OptimizedDataFrame()
        for name in self.column_names:
            result.add_column(name, new if name == column_name else self.column(name))
        return result

    def _map_column(self, column_name, make):
        """`make(col(column_name))` evaluated in one call -> the frame with that column replaced.  Errors before any device
        call: ColumnNotFound, ColumnTypeMismatch for a String or Boolean column (as rank and describe)."""
        self._numeric(column_name)
        return self._replaced(column_name, self._eval_values(make(col(column_name))))

    def _zip_columns(self, col1, col2, result_name, make):
        """`make(col(col1), col(col2))` in one call -> the frame with the result appended as `result_name`; a name the
        frame already has is DuplicateColumnName, as the reference's DataFrame::add_column (dataframe/base.rs:143-145)."""
        self._numeric(col1), self._numeric(col2)
        if result_name in self.column_indices:
            raise DuplicateColumnName(result_name)
        new = self._eval_values(make(col(col1), col(col2)))
        result = OptimizedDataFrame()
        for name in self.column_names:
            result.add_column(name, self.column(name))
        return result.add_column(result_name, new)

    def with_column(self, name, expr):
        """A NEW frame with the value expression `expr` (col("a") * col("b") + 1.0, where(cond, a, b), ...) evaluated in ONE
        pandrs_hip_eval call as the Float64 column `name`: replaced in position when the frame has it, appended otherwise."""
        new = self._eval_values(expr)
        if name in self.column_indices:
            return self._replaced(name, new)
        result = OptimizedDataFrame()
        for n in self.column_names:
            result.add_column(n, self.column(n))
        return result.add_column(name, new)

    def mask_of(self, expr):
        """The condition `expr` (col("a") > col("b"), (x > 0) & ~y.isnan(), ...) per row, from one pandrs_hip_eval call ->
        list of bool."""
        views, program, is_mask = self._bind(expr)
        if not is_mask:
            raise InvalidValue("the expression is a value; a mask takes a condition")
        if self._row_count == 0:
            return []
        bits, _ = get_context().eval(views, self._row_count, program, out_device=False)
        return np.unpackbits(bits, count=self._row_count, bitorder="little").astype(bool).tolist()

    def filter_expr(self, expr):
        """The rows where the condition `expr` holds, every column kept, assembled as filter does: pandrs_hip_eval ->
        filter_indices on the device mask -> filter_gather per column; the mask does not visit the host."""
        views, program, is_mask = self._bind(expr)
        if not is_mask:
            raise InvalidValue("the expression is a value; a filter takes a condition")
        if self._row_count == 0:
            return self._empty_columns()
        bits, _ = get_context().eval(views, self._row_count, program, out_device=True)
        return self._compact((bits, None, L.BOOLBITS))[0]

    def add_scalar(self, column, value):
        """add_scalar (functions.rs:2819-2821): x + value, the column replaced (Float64)."""
        return self._map_column(column, lambda x: x + float(value))

    def sub_scalar(self, column, value):
        """sub_scalar (functions.rs:2827-2829): x - value."""
        return self._map_column(column, lambda x: x - float(value))

    def mul_scalar(self, column, value):
        """mul_scalar (functions.rs:2823-2825): x * value."""
        return self._map_column(column, lambda x: x * float(value))

    def div_scalar(self, column, value):
        """div_scalar (functions.rs:2831-2833): x / value."""
        return self._map_column(column, lambda x: x / float(value))

    def sqrt(self, column):
        """sqrt (functions.rs:2839-2841): x.sqrt(), correctly rounded; NaN for a negative cell."""
        return self._map_column(column, lambda x: x.sqrt())

    def col_add(self, col1, col2, result_name):
        """col_add (functions.rs:2851-2877): a + b appended as `result_name`."""
        return self._zip_columns(col1, col2, result_name, lambda a, b: a + b)

    def col_sub(self, col1, col2, result_name):
        """col_sub (functions.rs:2907-2933): a - b."""
        return self._zip_columns(col1, col2, result_name, lambda a, b: a - b)

    def col_mul(self, col1, col2, result_name):
        """col_mul (functions.rs:2879-2905): a * b."""
        return self._zip_columns(col1, col2, result_name, lambda a, b: a * b)

    def col_div(self, col1, col2, result_name):
        """col_div (functions.rs:2935-2960): a / b."""
        return self._zip_columns(col1, col2, result_name, lambda a, b: a / b)

    def add_columns(self, col1, col2, result_name):
        """add_columns (functions.rs:3890-3912): v1 + v2 appended as `result_name`."""
        return self._zip_columns(col1, col2, result_name, lambda a, b: a + b)

    def sub_columns(self, col1, col2, result_name):
        """sub_columns (functions.rs:3914-3936): v1 - v2."""
        return self._zip_columns(col1, col2, result_name, lambda a, b: a - b)

    def mul_columns(self, col1, col2, result_name):
        """mul_columns (functions.rs:3938-3960): v1 * v2."""
        return self._zip_columns(col1, col2, result_name, lambda a, b: a * b)

    def div_columns(self, col1, col2, result_name):
        """div_columns (functions.rs:3962-3984): v1 / v2."""
        return self._zip_columns(col1, col2, result_name, lambda a, b: a / b)

    def coalesce(self, col1, col2, result_name):
        """coalesce (functions.rs:3846-3868): v1.is_nan() ? v2 : v1 appended as `result_name`; a null cell counts as NaN."""
        return self._zip_columns(col1, col2, result_name, lambda a, b: where(a.isnan(), b, a))

    def abs(self, column):
        """abs (functions.rs:691-709): x.abs(), the column replaced."""
        return self._map_column(column, lambda x: x.abs())

    def abs_column(self, column):
        """abs_column (functions.rs:3713-3715, helpers/math_ops.rs:64-69)."""
        return self.abs(column)

    def round(self, column, decimals):
        """round (functions.rs:711-730): (x * f).round() / f with f = 10f64.powi(decimals), half away from zero; f is
        computed on the host the way powi does (the exact power, its reciprocal for negative decimals)."""
        decimals = int(decimals)
        f = 10.0 ** abs(decimals)
        if decimals < 0:
            f = 1.0 / f
        return self._map_column(column, lambda x: (x * f).round() / f)

    def round_column(self, column, decimals):
        """round_column (functions.rs:3717-3719, helpers/math_ops.rs:71-80)."""
        return self.round(column, decimals)

    def neg(self, column):
        """neg (functions.rs:3994-3996, helpers/math_ops.rs:82-87): -x."""
        return self._map_column(column, lambda x: -x)

    def floor(self, column):
        """floor (functions.rs:4069-4071, helpers/math_ops.rs:29-34)."""
        return self._map_column(column, lambda x: x.floor())

    def ceil(self, column):
        """ceil (functions.rs:4073-4075, helpers/math_ops.rs:36-41)."""
        return self._map_column(column, lambda x: x.ceil())

    def trunc(self, column):
        """trunc (functions.rs:4077-4079, helpers/math_ops.rs:43-48)."""
        return self._map_column(column, lambda x: x.trunc())

    def fract(self, column):
        """fract (functions.rs:4081-4083, helpers/math_ops.rs:50-55): x - x.trunc()."""
        return self._map_column(column, lambda x: x.fract())

    def reciprocal(self, column):
        """reciprocal (functions.rs:4085-4087, helpers/math_ops.rs:57-62): 1.0 / x."""
        return self._map_column(column, lambda x: 1.0 / x)

    def mod_column(self, column, divisor):
        """mod_column (functions.rs:3986-3988, helpers/math_ops.rs:89-94): x % divisor, C's fmod."""
        return self._map_column(column, lambda x: x % float(divisor))

    def floordiv(self, column, divisor):
        """floordiv (functions.rs:3990-3992, helpers/math_ops.rs:96-101): (x / divisor).floor()."""
        return self._map_column(column, lambda x: (x / float(divisor)).floor())

    def clip(self, column, lower=None, upper=None):
        """clip (functions.rs:237-252): x.max(lower) then .min(upper), either bound optional.  Through f64::max / f64::min a
        NaN cell clips TO THE BOUND.  The column is replaced (the reference's own add_column of the existing name fails with
        DuplicateColumnName; clip_lower / clip_upper show what is meant)."""
        def make(x):
            if lower is not None:
                x = x.max(float(lower))
            if upper is not None:
                x = x.min(float(upper))
            return x if lower is not None or upper is not None else x + lit(-0.0)      # (the identity, still one program)
        return self._map_column(column, make)

    def clip_lower(self, column, min):
        """clip_lower (functions.rs:3787-3805): x.max(min)."""
        return self._map_column(column, lambda x: x.max(float(min)))

    def clip_upper(self, column, max):
        """clip_upper (functions.rs:3807-3825): x.min(max)."""
        return self._map_column(column, lambda x: x.min(float(max)))

    def _cond_expr(self, condition):
        """The condition of where_cond / mask as an expression over one more BOOLBITS column: a list of bool, a BooleanColumn
        or a device mask (the bits of predicate(..., out_device=True)).  A wrong length raises InvalidValue
        (functions.rs:1082-1086)."""
        if isinstance(condition, BooleanColumn):
            length, view = condition.len(), condition.view()
        elif type(condition).__module__.startswith("torch"):
            length, view = self._row_count if condition.numel() == (self._row_count + 7) // 8 else -1, (condition, None, L.BOOLBITS)
        else:
            cond = np.asarray(condition, dtype=bool).reshape(-1)
            length, view = cond.shape[0], (np.packbits(cond, bitorder="little"), None, L.BOOLBITS)
        if length != self._row_count:
            raise InvalidValue("Condition length must match column length")
        return view

    def _where(self, column, condition, other, keep_where):
        c = self._numeric(column)
        cond = self._cond_expr(condition)
        if self._row_count == 0:
            return self._replaced(column, Float64Column([]))
        program = [(L.EVAL_COL, 0), (L.EVAL_COL, 1), (L.EVAL_CONST, float(other)), (L.EVAL_SELECT, 0)] if keep_where else \
                  [(L.EVAL_COL, 0), (L.EVAL_CONST, float(other)), (L.EVAL_COL, 1), (L.EVAL_SELECT, 0)]
        ctx = get_context()
        view, resident = c.view(), None
        if type(cond[0]).__module__.startswith("torch"):                 # the mask lives on the device: so does the column for this call
            view = resident = ctx.upload_column_n(c.data, c.null_mask, c.dtype, self._row_count)
        try:
            values, mask, _ = ctx.eval([cond, view], self._row_count, program, out_device=False)
        finally:
            if resident is not None:
                resident.release()
        new = Float64Column(np.asarray(values))
        new.null_mask = None if mask is None else np.asarray(mask)
        return self._replaced(column, new)

    def where_cond(self, column, condition, other):
        """where_cond (functions.rs:1079-1108): cond ? x : other per row, the column replaced.  `condition`: a list of bool,
        a BooleanColumn (a null condition is false) or a device mask from Context.predicate(..., out_device=True), which
        does not visit the host."""
        return self._where(column, condition, other, True)

    def mask(self, column, condition, other):
        """mask (functions.rs:1110-1139): cond ? other : x per row."""
        return self._where(column, condition, other, False)

    def fillna_zero(self, column):
        """fillna_zero (functions.rs:4097-4118): x.is_nan() ? 0.0 : x; a null cell counts as NaN."""
        return self._map_column(column, lambda x: where(x.isnan(), lit(0.0), x))

    def replace_inf(self, column, replacement):
        """replace_inf (functions.rs:4026-4049): x.is_infinite() ? replacement : x."""
        return self._map_column(column, lambda x: where(x.isinf(), lit(float(replacement)), x))

    def sign(self, column):
        """sign (functions.rs:3998-4014): 1 / -1 / 0 per row (0 for NaN and both zeros), -> list of int."""
        self._numeric(column)
        return [int(v) for v in self._eval_values(col(column).sign()).data]

    def normalize(self, column):
        """normalize (functions.rs:2316-2337): (x - min) / (max - min) with min / max over the cells that are not NaN
        (value_range, :2270-2282; the whole-column reduction, exact in any order), NaN stays NaN, -> list of float.
        InvalidValue where the reference raises it: no valid value, or a range of zero."""
        c = self._numeric(column)
        if c.len() == 0:
            raise InvalidValue("No valid values in column")
        st = get_context().column_stats(c.view(), c.len())
        lo, hi = float(st["min"]), float(st["max"])
        if lo > hi:                                                      # the fold identities: no cell that is not NaN
            raise InvalidValue("No valid values in column")
        rng = hi - lo
        if rng == 0.0:
            raise InvalidValue("Range is zero, cannot normalize")
        return self._eval_values((col(column) - lo) / rng).data.tolist()

    # -- joins (join.rs:32-73) -----------------------------------------------------------------------------
    def inner_join(self, other, left_on, right_on):
        return self._join_impl(other, left_on, right_on, JoinType.Inner)

    def left_join(self, other, left_on, right_on):
        return self._join_impl(other, left_on, right_on, JoinType.Left)

    def right_join(self, other, left_on, right_on):
        return self._join_impl(other, left_on, right_on, JoinType.Right)

    def outer_join(self, other, left_on, right_on):
        return self._join_impl(other, left_on, right_on, JoinType.Outer)

    def _join_impl(self, other, left_on, right_on, how):
        if left_on not in self.column_indices:
            raise ColumnNotFound(left_on)                     # join.rs:84-87
        if right_on not in other.column_indices:
            raise ColumnNotFound(right_on)                    # join.rs:89-92
        lcol, rcol = self.column(left_on), other.column(right_on)
        ctx = get_context()
        # dtype mismatch => ColumnTypeMismatch raised by the library (join.rs:98-104)
        li, ri = ctx.join_indices(lcol.view(), lcol.len(), rcol.view(), rcol.len(), int(how))
        result = OptimizedDataFrame()
        if len(li) == 0:
            # empty result: NON-KEY columns only, suffix decided against the LEFT frame (join.rs:227-284)
            for name in self.column_names:
                if name != left_on:
                    result.add_column(name, _empty_like(self.column(name)))
            for name in other.column_names:
                if name != right_on:
                    new = name + "_right" if name in self.column_indices else name
                    result.add_column(new, _empty_like(other.column(name)))
            return result
        g = _Gatherer(ctx, li, ri)
        for name in self.column_names:                        # left non-key columns (join.rs:290-361)
            if name != left_on:
                result.add_column(name, g.take(self.column(name), left=True))
        result.add_column(left_on, g.take_key(lcol, rcol))    # key: left value, else right (join.rs:364-472)
        for name in other.column_names:                       # right non-key columns (join.rs:475-552)
            if name != right_on:
                new = name + "_right" if name in result.column_indices else name
                result.add_column(new, g.take(other.column(name), left=False))
        return result


# ---------------------------------------------------------------- expressions over columns (pandrs_hip_eval)
_EXPR_ARITY = {L.EVAL_ADD: 2, L.EVAL_SUB: 2, L.EVAL_MUL: 2, L.EVAL_DIV: 2, L.EVAL_REM: 2, L.EVAL_MAX: 2, L.EVAL_MIN: 2,
               L.EVAL_GT: 2, L.EVAL_GE: 2, L.EVAL_LT: 2, L.EVAL_LE: 2, L.EVAL_EQ: 2, L.EVAL_NE: 2, L.EVAL_AND: 2, L.EVAL_OR: 2,
               L.EVAL_SELECT: 3}


class Expr:
    """A row-wise expression over the columns of a frame, built with col(), lit(), where() and the operators below, and
    evaluated by OptimizedDataFrame.with_column / mask_of / filter_expr in ONE device call (pandrs_hip_eval): every
    operation is the reference's Rust expression rounded on its own.  + - * / % (fmod) and unary - act on values; > >= <
    <= == != compare two values the IEEE way (not eq_value's EPSILON compare) and give a condition; & | ~ combine
    conditions.  A plain number stands for lit(number)."""
    __hash__ = None

    def __init__(self, op, arg=0.0, children=()):
        self.op, self.arg, self.children = op, arg, tuple(children)

    @staticmethod
    def _of(x):
        if isinstance(x, Expr):
            return x
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise InvalidValue("an expression takes expressions and numbers, got %r" % (x,))
        return Expr(L.EVAL_CONST, float(x))

    def _bin(self, op, other, swap=False):
        a, b = self, Expr._of(other)
        return Expr(op, children=(b, a) if swap else (a, b))

    def lower(self):
        """-> (the distinct column names in first-use order, the postfix program as (op, arg) pairs)."""
        names, program = [], []

        def walk(e):
            for c in e.children:
                walk(c)
            if e.op == L.EVAL_COL:
                if e.arg not in names:
                    names.append(e.arg)
                program.append((L.EVAL_COL, float(names.index(e.arg))))
            else:
                program.append((e.op, float(e.arg)))
        walk(self)
        return names, program

    def __add__(self, o): return self._bin(L.EVAL_ADD, o)
    def __radd__(self, o): return self._bin(L.EVAL_ADD, o, True)
    def __sub__(self, o): return self._bin(L.EVAL_SUB, o)
    def __rsub__(self, o): return self._bin(L.EVAL_SUB, o, True)
    def __mul__(self, o): return self._bin(L.EVAL_MUL, o)
    def __rmul__(self, o): return self._bin(L.EVAL_MUL, o, True)
    def __truediv__(self, o): return self._bin(L.EVAL_DIV, o)
    def __rtruediv__(self, o): return self._bin(L.EVAL_DIV, o, True)
    def __mod__(self, o): return self._bin(L.EVAL_REM, o)
    def __rmod__(self, o): return self._bin(L.EVAL_REM, o, True)
    def __neg__(self): return Expr(L.EVAL_NEG, children=(self,))
    def __abs__(self): return self.abs()
    def __gt__(self, o): return self._bin(L.EVAL_GT, o)
    def __ge__(self, o): return self._bin(L.EVAL_GE, o)
    def __lt__(self, o): return self._bin(L.EVAL_LT, o)
    def __le__(self, o): return self._bin(L.EVAL_LE, o)
    def __eq__(self, o): return self._bin(L.EVAL_EQ, o)
    def __ne__(self, o): return self._bin(L.EVAL_NE, o)
    def __and__(self, o): return self._bin(L.EVAL_AND, o)
    def __rand__(self, o): return self._bin(L.EVAL_AND, o, True)
    def __or__(self, o): return self._bin(L.EVAL_OR, o)
    def __ror__(self, o): return self._bin(L.EVAL_OR, o, True)
    def __invert__(self): return Expr(L.EVAL_NOT, children=(self,))

    def __bool__(self):
        raise InvalidValue("an expression has no truth value; combine conditions with & | ~")

    def abs(self): return Expr(L.EVAL_ABS, children=(self,))
    def floor(self): return Expr(L.EVAL_FLOOR, children=(self,))
    def ceil(self): return Expr(L.EVAL_CEIL, children=(self,))
    def trunc(self): return Expr(L.EVAL_TRUNC, children=(self,))
    def fract(self): return Expr(L.EVAL_FRACT, children=(self,))
    def sqrt(self): return Expr(L.EVAL_SQRT, children=(self,))
    def sign(self): return Expr(L.EVAL_SIGN, children=(self,))
    def isnan(self): return Expr(L.EVAL_ISNAN, children=(self,))
    def isinf(self): return Expr(L.EVAL_ISINF, children=(self,))
    def isfinite(self): return Expr(L.EVAL_ISFINITE, children=(self,))

    def round(self):
        """f64::round: half away from zero."""
        return Expr(L.EVAL_ROUND, children=(self,))

    def max(self, o):
        """f64::max: a NaN operand is ignored."""
        return self._bin(L.EVAL_MAX, o)

    def min(self, o):
        """f64::min: a NaN operand is ignored."""
        return self._bin(L.EVAL_MIN, o)

    def clip(self, lower, upper):
        """x.max(lower).min(upper), the reference's clip (functions.rs:237-245): a NaN clips to the bound."""
        return self.max(lower).min(upper)


def col(name):
    """The column `name` of the frame the expression is evaluated on."""
    return Expr(L.EVAL_COL, name)


def lit(value):
    """The constant `value` as f64."""
    return Expr._of(float(value))


def where(cond, a, b):
    """cond ? a : b per row; a and b are both values or both conditions."""
    return Expr(L.EVAL_SELECT, children=(Expr._of(cond), Expr._of(a), Expr._of(b)))


# ---------------------------------------------------------------- the window builder (dataframe/enhanced_window.rs)
class DataFrameRolling:
    """enhanced_window.rs:14-54: a rolling configuration.  window_size, then .min_periods(n), .center(bool) and
    .columns([names]), each returning the configuration.  (`closed` is accepted by the reference and never read.)"""

    def __init__(self, window_size):
        self.window_size = int(window_size)
        self._min_periods = None
        self._center = False
        self._columns = None

    def min_periods(self, min_periods):
        self._min_periods = int(min_periods)
        return self

    def center(self, center):
        self._center = bool(center)
        return self

    def columns(self, columns):
        self._columns = list(columns)
        return self


class DataFrameExpanding:
    """enhanced_window.rs:56-75: an expanding configuration: min_periods, then .columns([names])."""

    def __init__(self, min_periods):
        self._min_periods = int(min_periods)
        self._columns = None

    def columns(self, columns):
        self._columns = list(columns)
        return self


class _DataFrameWindowOps:
    """DataFrameRollingOps / DataFrameExpandingOps (enhanced_window.rs:246-425, :427-560): every operation returns a new
    frame: every column of this one, then a Float64Column "{column}_{operation}" per target column (:350, :404).  The
    targets are the configured columns, else every Int64 / Float64 column (:411-424).  Every error is raised before any
    device call: ColumnNotFound, ColumnTypeMismatch, InvalidValue, DuplicateColumnName."""

    def __init__(self, frame, config):
        self.frame = frame
        self.config = config

    def _spec(self):
        raise NotImplementedError

    def _targets(self):
        cols = self.config._columns
        if cols is not None:
            for name in cols:
                if name not in self.frame.column_indices:
                    raise ColumnNotFound(name)
            return list(cols)
        return [name for name in self.frame.column_names if self.frame.column(name).dtype in (L.I64, L.F64)]

    def _apply(self, operation, run, check=None):
        frame = self.frame
        targets = self._targets()
        names, seen = [], set(frame.column_indices)
        for name in targets:
            frame._window_column(name)
            self._validate()
            if check is not None:
                check()
            out_name = "%s_%s" % (name, operation)
            if out_name in seen:
                raise DuplicateColumnName(out_name)
            seen.add(out_name)
            names.append(out_name)
        n = frame.row_count()
        result = OptimizedDataFrame()
        for c in frame.column_names:
            result.add_column(c, frame.column(c))
        for name, out_name in zip(targets, names):
            values = np.asarray(run(frame.column(name).view(), n), np.float64) if n else np.empty(0)
            result.add_column(out_name, Float64Column(values))
        return result

    def _window(self, operation, op, ddof=1):
        if int(ddof) < 0:
            raise InvalidValue("ddof must be >= 0")
        kind, spec = self._spec()
        return self._apply(operation, lambda view, n: get_context().window(view, n, kind, op, ddof=int(ddof), out_device=False, **spec))

    def mean(self):
        return self._window("mean", L.WINDOW_MEAN)

    def sum(self):
        return self._window("sum", L.WINDOW_SUM)

    def std(self, ddof):
        return self._window("std", L.WINDOW_STD, ddof)

    def var(self, ddof):
        return self._window("var", L.WINDOW_VAR, ddof)

    def min(self):
        return self._window("min", L.WINDOW_MIN)

    def max(self):
        return self._window("max", L.WINDOW_MAX)

    def count(self):
        return self._window("count", L.WINDOW_COUNT)

    def median(self):
        """Rolling / Expanding::median (series/window.rs:298-315, :494-511) of every target column, on the device."""
        kind, spec = self._spec()
        return self._apply("median", lambda view, n: get_context().window_quantile(view, n, kind, median=True, out_device=False, **spec))

    def quantile(self, q):
        """Rolling / Expanding::quantile (series/window.rs:317-336, :513-532): sorted[min(round(q * (len-1)), len-1)].
        q outside [0, 1] (or NaN) is InvalidValue("Quantile must be between 0 and 1")."""
        q = float(q)

        def check():
            if not (0.0 <= q <= 1.0):
                raise InvalidValue("Quantile must be between 0 and 1")
        kind, spec = self._spec()
        return self._apply("quantile", lambda view, n: get_context().window_quantile(view, n, kind, median=False, q=q, out_device=False, **spec),
                           check)


class DataFrameRollingOps(_DataFrameWindowOps):
    def _validate(self):
        if self.config.window_size <= 0:
            raise InvalidValue("Window size must be greater than 0")            # series/window.rs:112-117
        if self.config._min_periods is not None and self.config._min_periods < 0:
            raise InvalidValue("min_periods must be >= 0")

    def _spec(self):
        c = self.config
        return L.WINDOW_KIND_ROLLING, {"window": c.window_size, "min_periods": c.window_size if c._min_periods is None else c._min_periods,
                                       "center": c._center}


class DataFrameExpandingOps(_DataFrameWindowOps):
    def _validate(self):
        if self.config._min_periods < 0:
            raise InvalidValue("min_periods must be >= 0")

    def _spec(self):
        return L.WINDOW_KIND_EXPANDING, {"min_periods": self.config._min_periods}


def _empty_like(col):
    if isinstance(col, Int64Column):
        return Int64Column([])
    if isinstance(col, Float64Column):
        return Float64Column([])
    if isinstance(col, StringColumn):
        return StringColumn([])
    return BooleanColumn([])


class _Gatherer:
    """Column gathers of join_impl on the device: misses / nulls become 0 / 0.0 / "" / false and the
    result columns carry NO null mask (join.rs:304-307, :319-322)."""

    def __init__(self, ctx, li, ri):
        import torch
        self.torch = torch
        self.ctx = ctx
        self.dev = "cuda:%d" % ctx.device
        up = lambda a: a.to(self.dev) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.li, self.ri = up(li), up(ri)

    def _up(self, a):
        if a is None:
            return None
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _gather(self, col, idx):
        fill = GLOBAL_STRING_POOL.get_or_insert("") if col.dtype == L.U32CODE else 0
        if col.len() == 0:
            n = idx.numel()
            return {L.I64: np.zeros(n, np.int64), L.F64: np.zeros(n, np.float64),
                    L.U32CODE: np.full(n, fill, np.uint32), L.BOOLBITS: np.zeros(n, np.uint8)}[col.dtype]
        out = self.ctx.gather(self._up(col.data), self._up(col.null_mask), idx, fill, col.dtype).cpu().numpy()
        return out.view(np.uint32) if col.dtype == L.U32CODE else out

    @staticmethod
    def _wrap(col, arr):
        if col.dtype == L.I64:
            return Int64Column(arr)
        if col.dtype == L.F64:
            return Float64Column(arr)
        if col.dtype == L.U32CODE:
            return StringColumn.from_codes(arr)
        return BooleanColumn(None, _bits=np.packbits(arr.astype(bool), bitorder="little"), _length=len(arr))

    def take(self, col, left):
        return self._wrap(col, self._gather(col, self.li if left else self.ri))

    def take_key(self, lcol, rcol):
        a = self._gather(lcol, self.li)
        b = self._gather(rcol, self.ri)
        from_left = (self.li >= 0).cpu().numpy()
        return self._wrap(lcol, np.where(from_left, a, b))


# ---------------------------------------------------------------------------------------------- GroupBy
class GroupBy:
    """GroupBy<'a> (group/types.rs:46-55).  Aggregations run on the device straight from the
    columns; the row-index map `groups` (a pub field in the reference, types.rs:52) is built on the
    device too, but only when something reads it (closures: filter / custom aggregations)."""

    def __init__(self, df, group_by_columns, create_multi_index=False):
        self.df = df
        self.group_by_columns = group_by_columns
        self.create_multi_index = create_multi_index
        self._groups = None
        self._grouping = None       # (context, its grouping_token) after this GroupBy's own groupby_indices

    def _group_rows(self, null_string="NULL"):
        """{tuple(key strings) -> ascending row indices (numpy)} from pandrs_hip_groupby_indices."""
        key_cols = [self.df.column(k) for k in self.group_by_columns]
        cells, nulls, off, rows = get_context().groupby_indices([k.view() for k in key_cols], self.df.row_count())
        strs = [_key_strings(k.dtype, cells[i], nulls[i], null_string) for i, k in enumerate(key_cols)]
        return {key: rows[off[g]:off[g + 1]] for g, key in enumerate(zip(*strs))}

    @property
    def groups(self):
        """HashMap<Vec<String>, Vec<usize>> of the reference (grouping.rs:62-104)."""
        if self._groups is None:
            self._groups = {k: v.tolist() for k, v in self._group_rows().items()}
        return self._groups

    def _values(self, column, rows):
        """The group's non-null values of a numeric column as f64 (aggregation.rs:440-455)."""
        col = self.df.column(column)
        if col.dtype not in (L.I64, L.F64):
            raise OperationFailed(L.ERR_OPERATION_FAILED, "column '%s' is not numeric" % column)
        out = []
        for r in rows:
            v = col.get(r)
            if v is not None:
                out.append(float(v))
        return out

    def aggregate_custom(self, aggregations):
        """aggregations: iterable of (column, fn(list[float]) -> float, result_name)
        (CustomAggregation, types.rs:58-67; aggregate_custom, aggregation.rs:391-497): the closure
        runs on the host over the group's non-null values (Int64 cast to f64), groups from the device."""
        aggregations = list(aggregations)
        for column, fn, _ in aggregations:
            if fn is None:
                raise OperationFailed(L.ERR_OPERATION_FAILED,
                                      "Custom aggregation function is required for AggregateOp::Custom")
            if column not in self.df.column_indices:
                raise ColumnNotFound(column)
        result = OptimizedDataFrame()
        groups = self.groups
        for i, name in enumerate(self.group_by_columns):
            result.add_column(name, StringColumn([k[i] for k in groups]))
        for column, fn, result_name in aggregations:
            result.add_column(result_name, Float64Column([float(fn(self._values(column, rows))) for rows in groups.values()]))
        return result

    def custom(self, column, result_name, func):          # operations.rs:606
        return self.aggregate_custom([(column, func, result_name)])

    par_custom = custom
    par_aggregate_custom = aggregate_custom

    def filter(self, filter_fn):
        """operations.rs:51-74: keep the rows of the groups whose sub-frame passes filter_fn."""
        keep = [np.asarray(rows, np.int64) for rows in self.groups.values()
                if filter_fn(self.df.filter_by_indices(rows))]
        return self.df.filter_by_indices(np.concatenate(keep) if keep else np.zeros(0, np.int64))

    par_filter = filter

    def transform(self, transform_fn):
        """operations.rs:132-276: transform_fn(group sub-frame) -> frame, for every group; the results are
        concatenated column by column after the first result's schema (columns matched by POSITION, a
        column of another type contributes nothing, like the reference's `if let Some(Column::X(..))`)."""
        outs = [transform_fn(self.df.filter_by_indices(rows)) for rows in self.groups.values()]
        result = OptimizedDataFrame()
        if not outs:
            return result
        template = outs[0]
        for ci, tcol in enumerate(template.columns):
            values = []
            for df in outs:
                if ci < len(df.columns) and type(df.columns[ci]) is type(tcol):
                    col = df.columns[ci]
                    values.extend(col.get(i) for i in range(col.len()))
            nulls = [v is None for v in values]
            fill = {Int64Column: 0, Float64Column: 0.0, StringColumn: "", BooleanColumn: False}[type(tcol)]
            data = [fill if v is None else v for v in values]
            result.add_column(template.column_names[ci], type(tcol)(data, nulls if any(nulls) else None))
        return result

    par_transform = transform

    # -- folds and lags within the groups (pandrs_hip_grouped): no closure, no sub-frames ---------------------------------
    def _grouped(self, column_name, op, periods=0):
        """One pandrs_hip_grouped call -> (values as a host array, null bitmap or None), aligned with the frame's rows.  The
        grouping is built once and reused while the context still retains it (its grouping_token is this GroupBy's).  Errors
        before any device call, as the frame-level methods: ColumnNotFound, ColumnTypeMismatch for a String or Boolean column,
        InvalidValue for negative periods of diff / pct_change; an empty frame gives an empty result."""
        col = None if column_name is None else self.df._numeric(column_name)
        periods = int(periods)
        if op in (L.GROUPED_DIFF, L.GROUPED_PCT_CHANGE) and periods < 0:
            raise InvalidValue("periods must not be negative, got %d" % periods)
        n = self.df.row_count()
        if n == 0:
            return np.empty(0, np.int64 if op in (L.GROUPED_CUM_COUNT, L.GROUPED_ROW_NUMBER) else np.float64), None
        ctx = get_context()
        if self._grouping is None or self._grouping[0] is not ctx or self._grouping[1] != ctx.grouping_token:
            ctx.groupby_indices_compute([self.df.column(k).view() for k in self.group_by_columns], n)
            self._grouping = (ctx, ctx.grouping_token)
        values, mask, _ = ctx.grouped(None if col is None else col.view(), n, op, periods, out_device=False)
        return np.asarray(values), mask

    def cumsum(self, column):
        """The running sum of `column` within each group, in row order, -> list of float aligned with the frame's rows
        (OptimizedDataFrame.cumsum per group; pandrs_hip.h: every group's prefix is folded from its own cells)."""
        return self._grouped(column, L.GROUPED_CUM_SUM)[0].tolist()

    def cummax(self, column):
        """OptimizedDataFrame.cummax within each group, -> list of float."""
        return self._grouped(column, L.GROUPED_CUM_MAX)[0].tolist()

    def cummin(self, column):
        """OptimizedDataFrame.cummin within each group, -> list of float."""
        return self._grouped(column, L.GROUPED_CUM_MIN)[0].tolist()

    def cumcount(self, column):
        """OptimizedDataFrame.cumcount within each group: the group's rows so far that are neither NaN nor null, -> list of int."""
        return [int(v) for v in self._grouped(column, L.GROUPED_CUM_COUNT)[0]]

    def row_number(self):
        """The position of every row within its group (0 for the group's first row), null or not, -> list of int."""
        return [int(v) for v in self._grouped(None, L.GROUPED_ROW_NUMBER)[0]]

    def shift(self, column, periods):
        """OptimizedDataFrame.shift within each group: a row takes the cell `periods` rows earlier in its group, -> list of
        float or None (no source row in the group, or a null one)."""
        values, mask = self._grouped(column, L.GROUPED_SHIFT, periods)
        out = values.tolist()
        if mask is not None:
            for i in np.flatnonzero(np.unpackbits(mask, bitorder="little")[:len(out)]):
                out[i] = None
        return out

    def diff(self, column, periods):
        """OptimizedDataFrame.diff within each group, NaN for a group's first `periods` rows, -> list of float."""
        return self._grouped(column, L.GROUPED_DIFF, periods)[0].tolist()

    def pct_change(self, column, periods):
        """OptimizedDataFrame.pct_change within each group, -> list of float."""
        return self._grouped(column, L.GROUPED_PCT_CHANGE, periods)[0].tolist()

    def aggregate(self, aggregations):
        """aggregations: iterable of (column, AggregateOp, alias)  (aggregation.rs:763-871)."""
        aggregations = [(c, AggregateOp(int(op)), alias) for c, op, alias in aggregations]
        for col_name, _, _ in aggregations:
            if col_name not in self.df.column_indices:
                raise ColumnNotFound(col_name)                # aggregation.rs:770-774
        key_cols = [self.df.column(k) for k in self.group_by_columns]
        val_names = []
        for col_name, _, _ in aggregations:
            if col_name not in val_names:
                val_names.append(col_name)
        vals = [self.df.column(n).view() for n in val_names]
        specs = [(val_names.index(c), int(op)) for c, op, _ in aggregations]
        ctx = get_context()
        kc, kn, oa = ctx.groupby_agg([k.view() for k in key_cols], self.df.row_count(), vals, specs)
        result = OptimizedDataFrame()
        key_strings = [_key_strings(k.dtype, kc[i], kn[i]) for i, k in enumerate(key_cols)]
        if self.create_multi_index:
            # > 1 key with the multi-index option: no key columns, a StringMultiIndex of tuples instead
            # (aggregation.rs:812-853)
            result.multi_index = list(zip(*key_strings))
            result.multi_index_names = list(self.group_by_columns)
        else:
            # key columns as strings (aggregation.rs:856-860; their relative order is HashMap order in
            # the reference, group_by order here), then one Float64Column per alias in request order (:863-867)
            for name, strs in zip(self.group_by_columns, key_strings):
                result.add_column(name, StringColumn(strs))
        seen = {}
        for a, (_, _, alias) in enumerate(aggregations):
            seen[alias] = a          # the reference keeps one Vec per alias in a HashMap: last writer wins
        for a, (_, _, alias) in enumerate(aggregations):
            if alias in result.column_indices:
                raise DuplicateColumnName(alias)
            result.add_column(alias, Float64Column(oa[seen[alias]]))
        return result

    def agg(self, aggs):
        """[(column, op)] -> aliases "{col}_{op}" (operations.rs:498-521)."""
        return self.aggregate([(c, op, "%s_%s" % (c, _OP_NAME[AggregateOp(int(op))])) for c, op in aggs])

    par_aggregate = aggregate        # G6: the reference's parallel variant has a known row race
    par_agg = agg

    def _short(self, column, op):
        return self.aggregate([(column, op, "%s_%s" % (column, _OP_NAME[op]))])

    def sum(self, column):
        return self._short(column, AggregateOp.Sum)

    def mean(self, column):
        return self._short(column, AggregateOp.Mean)

    def min(self, column):
        return self._short(column, AggregateOp.Min)

    def max(self, column):
        return self._short(column, AggregateOp.Max)

    def count(self, column):
        return self._short(column, AggregateOp.Count)

    def std(self, column):
        return self._short(column, AggregateOp.Std)

    def var(self, column):
        return self._short(column, AggregateOp.Var)

    def median(self, column):
        return self._short(column, AggregateOp.Median)

    def first(self, column):
        return self._short(column, AggregateOp.First)

    def last(self, column):
        return self._short(column, AggregateOp.Last)

    def nunique(self, column):       # legacy GroupBy::nunique, src/dataframe/groupby.rs:386-393, alias "{col}_nunique"
        return self._short(column, AggregateOp.Nunique)

    # ---- GroupByJitExt (src/optimized/jit/groupby.rs:68-290).  The reference wraps fixed closures in
    # CustomAggregation and runs them through aggregate_custom over each group's non-null f64 values:
    # Kahan sum / mean / std, plain min / max folds, and the chunked "parallel" variants.  The same
    # quantities come out of the device aggregates; what differs from the AggregateOp path is only the
    # value for a group WITHOUT non-null values (min / max folds stay at +-inf instead of 0.0) and the
    # parallel std being the POPULATION std from E[x^2] - E[x]^2 (jit/parallel.rs:222-233).  Kahan and the
    # device's sums agree to ~1e-13 relative on benign data; tests compare with the closures themselves.
    def _jit(self, column, result_name, op, fix=None):
        col = self.df.column(column) if column in self.df.column_indices else None
        if col is None:
            raise ColumnNotFound(column)
        if col.dtype not in (L.I64, L.F64):
            raise OperationFailed(L.ERR_OPERATION_FAILED, "column '%s' is not numeric" % column)
        key_cols = [self.df.column(k) for k in self.group_by_columns]
        n = self.df.row_count()
        vals = [col.view()]
        specs = [(0, int(op)), (0, int(AggregateOp.Count))]
        if col.null_mask is not None:        # nulls per group: the sum of an indicator column
            ind = np.unpackbits(col.null_mask, bitorder="little")[:n].astype(np.int64)
            vals.append((ind, None, L.I64))
            specs.append((1, int(AggregateOp.Sum)))
        kc, kn, oa = get_context().groupby_agg([k.view() for k in key_cols], n, vals, specs)
        nn = oa[1] - (oa[2] if len(specs) == 3 else 0.0)          # non-null values per group
        out = fix(oa[0], nn) if fix else oa[0]
        result = OptimizedDataFrame()
        for i, (name, k) in enumerate(zip(self.group_by_columns, key_cols)):
            result.add_column(name, StringColumn(_key_strings(k.dtype, kc[i], kn[i])))
        result.add_column(result_name, Float64Column(np.asarray(out, np.float64)))
        return result

    def sum_jit(self, column, result_name):                # jit/groupby.rs:69-96
        return self._jit(column, result_name, AggregateOp.Sum)

    def mean_jit(self, column, result_name):               # :98-128, empty -> 0.0
        return self._jit(column, result_name, AggregateOp.Mean)

    def std_jit(self, column, result_name):                # :130-172, n <= 1 -> 0.0, n - 1 denominator
        return self._jit(column, result_name, AggregateOp.Std)

    def var_jit(self, column, result_name):
        return self._jit(column, result_name, AggregateOp.Var)

    def min_jit(self, column, result_name):                # :174-190, fold from +inf: empty stays +inf
        return self._jit(column, result_name, AggregateOp.Min, lambda v, nn: np.where(nn == 0, np.inf, v))

    def max_jit(self, column, result_name):                # :192-208
        return self._jit(column, result_name, AggregateOp.Max, lambda v, nn: np.where(nn == 0, -np.inf, v))

    def parallel_sum_jit(self, column, result_name, config=None):     # :210-228 (Kahan per chunk + Kahan combine)
        return self._jit(column, result_name, AggregateOp.Sum)

    def parallel_mean_jit(self, column, result_name, config=None):    # :230-247, count 0 -> 0.0
        return self._jit(column, result_name, AggregateOp.Mean)

    def parallel_std_jit(self, column, result_name, config=None):     # :249-266 -> parallel_std_f64_value
        def population(v, nn):                                        # sample variance * (n - 1) / n, n <= 1 -> 0.0
            return np.sqrt(np.where(nn > 1, v * (nn - 1) / np.maximum(nn, 1), 0.0))
        return self._jit(column, result_name, AggregateOp.Var, population)

    def aggregate_jit(self, column, func, result_name):               # :268-290: any closure -> host custom path
        return self.aggregate_custom([(column, func, result_name)])

    # operations.rs:550-594: the par_* shortcuts share the exact path (see par_aggregate above)
    par_sum, par_mean, par_min, par_max, par_count = sum, mean, min, max, count
    par_std, par_var, par_median = std, var, median


# ---------------------------------------------------------------------------------------------- LazyFrame
class LazyFrame:
    """LazyFrame (lazy.rs:98-170): the Select, Filter, Aggregate and Join arms, executed in plan order (lazy.rs:172-425).
    Select is OptimizedDataFrame.select, Filter is par_filter (lazy.rs:175-182).  The Map and Sort arms are not mirrored:
    the reference's Sort arm (lazy.rs:426-...) orders rows by each value's formatted string (so 10 sorts before 9),
    which is a separate piece of work."""

    def __init__(self, df):
        self.source = df
        self.operations = []

    @classmethod
    def new(cls, df):
        return cls(df)

    def select(self, columns):
        self.operations.append(("select", [columns] if isinstance(columns, str) else list(columns)))
        return self

    def filter(self, condition):
        self.operations.append(("filter", condition))
        return self

    def aggregate(self, group_by, aggregations):
        self.operations.append(("aggregate", list(group_by), list(aggregations)))
        return self

    def join(self, right, left_on, right_on, join_type):
        self.operations.append(("join", right, left_on, right_on, JoinType(int(join_type))))
        return self

    def execute(self):
        df = self.source
        ops = list(self.operations)
        i = 0
        while i < len(ops):
            op = ops[i]
            i += 1
            if op[0] == "select":
                df = df.select(op[1])                                 # lazy.rs:175-178
            elif op[0] == "filter":
                df = df.par_filter(op[1])                             # lazy.rs:179-182
            elif op[0] == "aggregate":
                _, group_by, aggregations = op
                for _, agg_op, _ in aggregations:             # lazy.rs:377-382: only these five ops
                    if AggregateOp(int(agg_op)) not in (AggregateOp.Sum, AggregateOp.Mean, AggregateOp.Min,
                                                        AggregateOp.Max, AggregateOp.Count):
                        raise OperationFailed(L.ERR_OPERATION_FAILED,
                                              "Aggregation operation %s is not supported" % AggregateOp(int(agg_op)).name)
                # the arm builds its result inline and never a multi-index: key columns always (lazy.rs:390-394;
                # tests/optimized_groupby_test.rs:184 asserts 3 columns for two keys)
                df = df.group_by_with_options(group_by, False).aggregate(aggregations)
            else:
                _, right, left_on, right_on, jt = op
                # Join(Inner) immediately followed by Aggregate([g], [(v, Sum, alias)]) — lazy.rs:405-425 then :186 — with v a
                # left column and g a right column is BASELINE config 5: one fused device operator
                # (pandrs_hip_join_groupby_sum), the joined rows are never materialised
                if jt == JoinType.Inner and i < len(ops) and ops[i][0] == "aggregate":
                    fused = _fused_join_groupby_sum(df, right, left_on, right_on, ops[i][1], ops[i][2])
                    if fused is not None:
                        df = fused
                        i += 1
                        continue
                df = df._join_impl(right, left_on, right_on, jt)     # lazy.rs:405-425
        return df


def _fused_join_groupby_sum(left, right, left_on, right_on, group_by, aggregations):
    """The shape test of hip_shim.rs `lazy_join_groupby_sum_hip` (same conditions, same result frame); None = not
    that shape, the two arms run one after the other."""
    if len(group_by) != 1 or len(aggregations) != 1 or AggregateOp(int(aggregations[0][1])) != AggregateOp.Sum:
        return None
    group_col, (value_col, _, alias) = group_by[0], aggregations[0]
    if left_on not in left.column_indices or right_on not in right.column_indices:
        return None                                          # the join arm raises ColumnNotFound
    if value_col == left_on or not left.contains_column(value_col) or left.contains_column(group_col):
        return None
    if group_col.endswith("_right") and left.contains_column(group_col[:-6]) and right.contains_column(group_col[:-6]):
        right_name = group_col[:-6]                          # join.rs:478-482
    elif right.contains_column(group_col):
        right_name = group_col
    else:
        return None
    if right_name == right_on:
        return None
    lk, lv, rk, rg = left.column(left_on), left.column(value_col), right.column(right_on), right.column(right_name)
    if lk.dtype != rk.dtype or lv.dtype not in (L.I64, L.F64) or rg.dtype == L.BOOLBITS or rg.null_mask is not None:
        return None
    kc, kn, sums = get_context().join_groupby_sum(lk.view(), lv.view(), left.row_count(), rk.view(), rg.view(), right.row_count())
    result = OptimizedDataFrame()
    result.add_column(group_col, StringColumn(_key_strings(rg.dtype, kc[0], kn[0])))
    result.add_column(alias, Float64Column(sums[0]))
    return result
