"""The reference's whole-column shape statistics restated in pure Python, line by line: PandasCompatExt::skew / kurtosis
(src/dataframe/pandas_compat/functions.rs:1617-1665), sem / mad / prod / describe_column / geometric_mean / harmonic_mean / iqr /
cv / percentile_value / trimmed_mean (helpers/aggregations.rs:8-225), var_column / std_column (functions.rs:3571-3588), zscore
(:2284-2314), range / abs_sum (:4207-4224) and the per-frame lists (:934-1022, :1583-1615).  A column is a float64 array whose
null cells are NaN already (values_of); every function filters `!v.is_nan()` itself, as the reference does.

Every sum is Rust's sequential fold: `iter().sum::<f64>()` starts at -0.0, `product()` and `fold(1.0, ..)` at 1.0, f64::min /
f64::max from +inf / -inf.  powi(2) / powi(3) / powi(4) are d * d, (d * d) * d and (d * d) * (d * d), what llvm.powi expands to.

fields(valid)           the fields of pandrs_hip_moments_stats by those folds (the struct the device returns)
at_frac_n / at_frac_n1 / median_of / trimmed_slice   the four index rules over a sorted list
order_stats(values, ops)   what pandrs_hip_order_stats returns
"""
import math

import numpy as np

NAN = math.nan
EPSILON = 2.0 ** -52            # f64::EPSILON
WANT_CENTRAL, WANT_LOG, WANT_RECIP, WANT_PROD = 1, 2, 4, 8
AT_FRAC_N, AT_FRAC_N1, MEDIAN, TRIMMED_MEAN = range(4)


def values_of(data, null=None):
    """The cells as f64 (`v as f64` for integers), null cells as NaN."""
    v = np.asarray(data).astype(np.float64)
    if null is not None:
        v = v.copy()
        v[np.asarray(null, bool)] = np.nan
    return v


def valid_of(values):
    return [float(v) for v in np.asarray(values, np.float64) if not math.isnan(v)]


def rsum(terms):
    s = -0.0                    # Rust's Sum for f64 starts at -0.0
    for t in terms:
        s += t
    return s


def rprod(terms):
    p = 1.0
    for t in terms:
        p *= t
    return p


def _div(a, b):
    """IEEE division: Python raises on a zero divisor."""
    if b == 0.0:
        if a == 0.0 or math.isnan(a):
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _min(a, b):                 # f64::min
    return b if math.isnan(a) else a if math.isnan(b) else min(a, b)


def _max(a, b):
    return b if math.isnan(a) else a if math.isnan(b) else max(a, b)


def fold_min(valid):
    m = math.inf
    for v in valid:
        m = _min(m, v)
    return m


def fold_max(valid):
    m = -math.inf
    for v in valid:
        m = _max(m, v)
    return m


def _ln(x):
    return math.inf if math.isinf(x) else math.log(x)


def fields(values, want=WANT_CENTRAL | WANT_LOG | WANT_RECIP | WANT_PROD, mean=None):
    """pandrs_hip_moments_stats by sequential folds.  `mean`: take the central sums around this value instead of sum / count
    (the GPU tests pass the device's own mean, so that they check the fold and not the conditioning)."""
    valid = valid_of(values)
    n = len(valid)
    s = rsum(valid)
    f = {"count": n, "count_pos": sum(1 for v in valid if v > 0.0), "count_nonzero": sum(1 for v in valid if v != 0.0),
         "sum": s, "abs_sum": rsum(abs(v) for v in valid), "min": fold_min(valid), "max": fold_max(valid),
         "mean": _div(s, float(n))}
    m = f["mean"] if mean is None else mean
    central = bool(want & WANT_CENTRAL)
    f["m2"] = rsum((v - m) * (v - m) for v in valid) if central else NAN
    f["m3"] = rsum(((v - m) * (v - m)) * (v - m) for v in valid) if central else NAN
    f["m4"] = rsum(((v - m) * (v - m)) * ((v - m) * (v - m)) for v in valid) if central else NAN
    f["abs_dev"] = rsum(abs(v - m) for v in valid) if central else NAN
    f["log_sum"] = rsum(_ln(v) for v in valid if v > 0.0) if want & WANT_LOG else NAN
    f["recip_sum"] = rsum(1.0 / v for v in valid if v != 0.0) if want & WANT_RECIP else NAN
    f["prod"] = rprod(valid) if want & WANT_PROD else NAN
    return f


def terms(values, mean):
    """{field: the list of terms t_i its sum folds}, central terms around `mean`: for the tests' error bounds."""
    valid = valid_of(values)
    d = [v - mean for v in valid]
    return {"sum": valid, "abs_sum": [abs(v) for v in valid], "m2": [x * x for x in d], "m3": [(x * x) * x for x in d],
            "m4": [(x * x) * (x * x) for x in d], "abs_dev": [abs(x) for x in d], "log_sum": [_ln(v) for v in valid if v > 0.0],
            "recip_sum": [1.0 / v for v in valid if v != 0.0]}


# ---- the public methods, each the reference's expression with its early returns ---------------------------------------------------
def _sqrt(x):
    return NAN if math.isnan(x) or x < 0.0 else math.sqrt(x)


def _variance_terms(valid):
    n = float(len(valid))
    mean = rsum(valid) / n
    return n, mean, rsum((v - mean) * (v - mean) for v in valid)


def skew(values):                                   # functions.rs:1617-1640
    valid = valid_of(values)
    if len(valid) < 3:
        return NAN
    n, mean, ss = _variance_terms(valid)
    std_dev = _sqrt(ss / n)
    if std_dev == 0.0:
        return NAN
    m3 = rsum(((v - mean) * (v - mean)) * (v - mean) for v in valid) / n
    skewness = _div(m3, (std_dev * std_dev) * std_dev)
    adjustment = _sqrt(n * (n - 1.0)) / (n - 2.0)
    return skewness * adjustment


def kurtosis(values):                               # functions.rs:1642-1665
    valid = valid_of(values)
    if len(valid) < 4:
        return NAN
    n, mean, ss = _variance_terms(valid)
    std_dev = _sqrt(ss / n)
    if std_dev == 0.0:
        return NAN
    m4 = rsum(((v - mean) * (v - mean)) * ((v - mean) * (v - mean)) for v in valid) / n
    kurt = _div(m4, (std_dev * std_dev) * (std_dev * std_dev)) - 3.0
    return ((n - 1.0) / ((n - 2.0) * (n - 3.0))) * ((n + 1.0) * kurt + 6.0)


def var_column(values, ddof):                       # functions.rs:3571-3584
    valid = valid_of(values)
    if len(valid) <= ddof:
        return NAN
    n, _, ss = _variance_terms(valid)
    return ss / (n - float(ddof))


def std_column(values, ddof):                       # :3586-3588
    return _sqrt(var_column(values, ddof))


def sem(values, ddof):                              # aggregations.rs:8-23
    valid = valid_of(values)
    if len(valid) <= ddof:
        return NAN
    n, _, ss = _variance_terms(valid)
    variance = ss / float(len(valid) - ddof)
    return _sqrt(variance) / math.sqrt(n)


def mad(values):                                    # aggregations.rs:26-39
    valid = valid_of(values)
    if not valid:
        return NAN
    mean = rsum(valid) / float(len(valid))
    return rsum(abs(v - mean) for v in valid) / float(len(valid))


def prod(values):                                   # aggregations.rs:42-51
    valid = valid_of(values)
    return rprod(valid) if valid else NAN


def value_span(values):                             # range, functions.rs:4207-4219
    valid = valid_of(values)
    return fold_max(valid) - fold_min(valid) if valid else NAN


def abs_sum(values):                                # functions.rs:4221-4224
    return rsum(abs(v) for v in valid_of(values))


def cv(values):                                     # aggregations.rs:162-181
    valid = valid_of(values)
    if not valid:
        return NAN
    n, mean, ss = _variance_terms(valid)
    if abs(mean) < EPSILON:
        return NAN
    return _sqrt(ss / max(n - 1.0, 1.0)) / abs(mean)


def geometric_mean(values):                         # aggregations.rs:108-122
    valid = [v for v in valid_of(values) if v > 0.0]
    if not valid:
        return NAN
    x = rsum(_ln(v) for v in valid) / float(len(valid))
    return math.inf if x > 709.782712893384 else math.exp(x)


def harmonic_mean(values):                          # aggregations.rs:125-139
    valid = [v for v in valid_of(values) if v != 0.0]
    if not valid:
        return NAN
    return _div(float(len(valid)), rsum(1.0 / v for v in valid))


# ---- the four index rules -----------------------------------------------------------------------------------------------------------
def _sorted(values):
    """sort_by(partial_cmp): stable, -0.0 and 0.0 tie.  The device orders -0.0 first (pandrs_hip.h), so ties of zeros are put in
    that order here; nothing else can differ."""
    return sorted(valid_of(values), key=lambda v: (v, 0 if math.copysign(1.0, v) < 0 else 1))


def _usize(x):                  # `as usize`: truncates, saturates at 0
    return 0 if x <= 0.0 else int(x)


def at_frac_n(s, a):            # aggregations.rs:87-89, :152-153: sorted.get((len as f64 * a) as usize).unwrap_or(NAN)
    i = _usize(float(len(s)) * a)
    return s[i] if i < len(s) else NAN


def at_frac_n1(s, a):           # :198
    if not s:
        return NAN
    i = _usize(float(len(s) - 1) * a)
    return s[i] if i < len(s) else NAN


def median_of(s):               # functions.rs:1604-1609
    if not s:
        return NAN
    mid = len(s) // 2
    return (s[mid - 1] + s[mid]) / 2.0 if len(s) % 2 == 0 else s[mid]


def trimmed_slice(s, a):        # aggregations.rs:217-218
    t = _usize(float(len(s)) * a)
    return s[t:len(s) - t]


def iqr(values):                                    # aggregations.rs:142-159
    s = _sorted(values)
    if len(s) < 2:
        return NAN
    return at_frac_n(s, 0.75) - at_frac_n(s, 0.25)


def percentile_value(values, q):                    # aggregations.rs:184-200
    if q < 0.0 or q > 1.0:
        return NAN
    return at_frac_n1(_sorted(values), q)


def trimmed_mean(values, trim_fraction):            # aggregations.rs:203-225
    if trim_fraction < 0.0 or trim_fraction >= 0.5:
        return NAN
    s = _sorted(values)
    if not s:
        return NAN
    trimmed = trimmed_slice(s, trim_fraction)
    if not trimmed:
        return NAN
    return rsum(trimmed) / float(len(trimmed))


def describe_column(values):                        # aggregations.rs:54-105
    valid = valid_of(values)
    if not valid:
        return {"count": 0.0, "mean": NAN, "std": NAN, "min": NAN, "max": NAN}
    n, mean, ss = _variance_terms(valid)
    s = _sorted(values)
    return {"count": n, "mean": mean, "std": _sqrt(ss / max(n - 1.0, 1.0)), "min": fold_min(valid), "max": fold_max(valid),
            "25%": at_frac_n(s, 0.25), "50%": s[len(s) // 2] if len(s) // 2 < len(s) else NAN, "75%": at_frac_n(s, 0.75)}


def zscore(values):                                 # functions.rs:2284-2314; ValueError where the reference returns Err
    valid = valid_of(values)
    if len(valid) < 2:
        raise ValueError("Need at least 2 values for z-score")
    n, mean, ss = _variance_terms(valid)
    std_dev = _sqrt(ss / (n - 1.0))
    if std_dev == 0.0:
        raise ValueError("Standard deviation is zero")
    return [NAN if math.isnan(v) else _div(float(v) - mean, std_dev) for v in np.asarray(values, np.float64)]


# ---- the per-frame lists: {name: values} in column order -> [(name, value)] --------------------------------------------------------
def sum_all(cols):                                  # functions.rs:934-943
    return [(k, rsum(valid_of(v))) for k, v in cols.items()]


def mean_all(cols):                                 # :944-957
    return [(k, rsum(valid_of(v)) / float(len(valid_of(v)))) for k, v in cols.items() if valid_of(v)]


def var_all(cols):                                  # :975-991
    return [(k, var_column(v, 1)) for k, v in cols.items() if len(valid_of(v)) > 1]


def std_all(cols):                                  # :958-974
    return [(k, _sqrt(x)) for k, x in var_all(cols)]


def min_all(cols):                                  # :992-1005
    return [(k, fold_min(valid_of(v))) for k, v in cols.items() if valid_of(v)]


def max_all(cols):                                  # :1006-1022
    return [(k, fold_max(valid_of(v))) for k, v in cols.items() if valid_of(v)]


def product_all(cols):                              # :1583-1595
    return [(k, rprod(valid_of(v))) for k, v in cols.items() if valid_of(v)]


def median_all(cols):                               # :1597-1615
    return [(k, median_of(_sorted(v))) for k, v in cols.items() if valid_of(v)]


# ---- what the device entry returns -------------------------------------------------------------------------------------------------
def order_stats(values, ops):
    """pandrs_hip_order_stats: ([result per (op, arg)], m).  The early returns for `a` included."""
    s = _sorted(values)
    out = []
    for op, a in ops:
        if op == AT_FRAC_N:
            out.append(at_frac_n(s, a) if s else NAN)
        elif op == AT_FRAC_N1:
            out.append(NAN if a < 0.0 or a > 1.0 else at_frac_n1(s, a))
        elif op == MEDIAN:
            out.append(median_of(s))
        elif op == TRIMMED_MEAN:
            if a < 0.0 or a >= 0.5 or not s:
                out.append(NAN)
            else:
                t = trimmed_slice(s, a)
                out.append(rsum(t) / float(len(t)) if t else NAN)
        else:
            raise ValueError("unknown op %r" % (op,))
    return out, len(s)
