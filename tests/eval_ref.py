"""A numpy twin of pandrs_hip_eval (include/pandrs_hip.h): the validator, the evaluation of a postfix program over whole
columns, the canonical NaN and the null rule.  test_eval_ref.py holds it against a per-row loop written with Python's math;
the GPU tests compare the library against it bit for bit."""
import numpy as np

I64, F64, U32CODE, BOOLBITS = 0, 1, 2, 3
INVALID_ARGUMENT, TYPE_MISMATCH = 1, 2
MAX_OPS, MAX_COLS, MAX_DEPTH = 64, 8, 8
CANON_NAN = 0x7FF8000000000000

NAMES = ["COL", "CONST", "ADD", "SUB", "MUL", "DIV", "REM", "MAX", "MIN", "NEG", "ABS", "FLOOR", "CEIL", "TRUNC", "ROUND", "FRACT",
         "SQRT", "SIGN", "GT", "GE", "LT", "LE", "EQ", "NE", "ISNAN", "ISINF", "ISFINITE", "AND", "OR", "NOT", "SELECT"]
OP = {name: i for i, name in enumerate(NAMES)}
BINARY_VALUE = [OP[k] for k in ("ADD", "SUB", "MUL", "DIV", "REM", "MAX", "MIN")]
UNARY_VALUE = [OP[k] for k in ("NEG", "ABS", "FLOOR", "CEIL", "TRUNC", "ROUND", "FRACT", "SQRT", "SIGN")]
COMPARE = [OP[k] for k in ("GT", "GE", "LT", "LE", "EQ", "NE")]
CLASSIFY = [OP[k] for k in ("ISNAN", "ISINF", "ISFINITE")]


class EvalError(Exception):
    def __init__(self, status, op_index, what):
        Exception.__init__(self, "op %s: %s" % (op_index, what))
        self.status, self.op_index = status, op_index


def pops_of(op):
    if op <= OP["CONST"]:
        return 0
    if op in BINARY_VALUE or op in COMPARE or op in (OP["AND"], OP["OR"]):
        return 2
    return 3 if op == OP["SELECT"] else 1


def check(dtypes, program):
    """-> (is_mask, depth); raises EvalError with the status pandrs_hip_eval_check returns."""
    if not 1 <= len(dtypes) <= MAX_COLS:
        raise EvalError(INVALID_ARGUMENT, None, "n_cols")
    if not 1 <= len(program) <= MAX_OPS:
        raise EvalError(INVALID_ARGUMENT, None, "n_ops")
    stack, depth = [], 0                    # True: a boolean
    for i, (op, arg) in enumerate(program):
        if not 0 <= op <= OP["SELECT"]:
            raise EvalError(INVALID_ARGUMENT, i, "bad opcode")
        pops = pops_of(op)
        if len(stack) < pops:
            raise EvalError(INVALID_ARGUMENT, i, "underflow")
        top = stack[len(stack) - pops:]
        if op == OP["COL"]:
            if not (0 <= arg < len(dtypes)) or arg != np.floor(arg):
                raise EvalError(INVALID_ARGUMENT, i, "bad column index")
            dt = dtypes[int(arg)]
            if dt not in (I64, F64, BOOLBITS):
                raise EvalError(TYPE_MISMATCH, i, "dtype")
            out = dt == BOOLBITS
        elif op == OP["CONST"]:
            out = False
        elif op in (OP["AND"], OP["OR"], OP["NOT"]):
            if not all(top):
                raise EvalError(INVALID_ARGUMENT, i, "a value where a boolean is expected")
            out = True
        elif op == OP["SELECT"]:
            if not top[0] or top[1] != top[2]:
                raise EvalError(INVALID_ARGUMENT, i, "SELECT types")
            out = top[1]
        else:
            if any(top):
                raise EvalError(INVALID_ARGUMENT, i, "a boolean where a value is expected")
            out = op in COMPARE or op in CLASSIFY
        del stack[len(stack) - pops:]
        if len(stack) >= MAX_DEPTH:
            raise EvalError(INVALID_ARGUMENT, i, "stack depth")
        stack.append(out)
        depth = max(depth, len(stack))
    if len(stack) != 1:
        raise EvalError(INVALID_ARGUMENT, len(program) - 1, "entries left")
    return stack[0], depth


def round_half_away(x):
    t = np.trunc(x)
    with np.errstate(invalid="ignore"):
        up = np.abs(x - t) >= 0.5           # x - trunc(x) is exact
    return np.where(up, t + np.copysign(1.0, x), t)


def unpack(bits, n):
    return np.unpackbits(np.asarray(bits, dtype=np.uint8), count=n, bitorder="little").astype(bool)


class Result:
    """values: float64 (every NaN canonical) and nulls (bool per row), or mask: bool per row; count: the set bits; zero_tie: a
    MAX / MIN met +0.0 and -0.0 in some row (Rust does not fix which comes back, neither does the library)."""


def evaluate(cols, n, program):
    """cols: (data, nulls, dtype) per column; data an int64 / float64 array or, for BOOLBITS, a bool array; nulls a bool array or
    None.  -> Result."""
    is_mask, _ = check([c[2] for c in cols], program)
    stack, named, tie = [], set(), False
    with np.errstate(all="ignore"):
        for op, arg in program:
            if op == OP["COL"]:
                data, nulls, dt = cols[int(arg)]
                named.add(int(arg))
                if dt == BOOLBITS:
                    v = np.asarray(data, dtype=bool)[:n].copy()
                    if nulls is not None:
                        v &= ~np.asarray(nulls, dtype=bool)[:n]
                else:
                    v = np.asarray(data)[:n].astype(np.float64)        # an int64 cell: round to nearest even, Rust's `as f64`
                    if nulls is not None:
                        v[np.asarray(nulls, dtype=bool)[:n]] = np.nan
                stack.append(v)
                continue
            if op == OP["CONST"]:
                stack.append(np.full(n, arg, dtype=np.float64))
                continue
            args = [stack.pop() for _ in range(pops_of(op))][::-1]
            a = args[0]
            b = args[1] if len(args) > 1 else None
            name = NAMES[op]
            if name == "ADD": r = a + b
            elif name == "SUB": r = a - b
            elif name == "MUL": r = a * b
            elif name == "DIV": r = a / b
            elif name == "REM": r = np.fmod(a, b)
            elif name in ("MAX", "MIN"):
                r = np.fmax(a, b) if name == "MAX" else np.fmin(a, b)
                tie = tie or bool(np.any((a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))))
            elif name == "NEG": r = -a
            elif name == "ABS": r = np.abs(a)
            elif name == "FLOOR": r = np.floor(a)
            elif name == "CEIL": r = np.ceil(a)
            elif name == "TRUNC": r = np.trunc(a)
            elif name == "ROUND": r = round_half_away(a)
            elif name == "FRACT": r = a - np.trunc(a)
            elif name == "SQRT": r = np.sqrt(a)
            elif name == "SIGN": r = np.where(a > 0, 1.0, np.where(a < 0, -1.0, 0.0))
            elif name == "GT": r = a > b
            elif name == "GE": r = a >= b
            elif name == "LT": r = a < b
            elif name == "LE": r = a <= b
            elif name == "EQ": r = a == b
            elif name == "NE": r = a != b
            elif name == "ISNAN": r = np.isnan(a)
            elif name == "ISINF": r = np.isinf(a)
            elif name == "ISFINITE": r = np.isfinite(a)
            elif name == "AND": r = a & b
            elif name == "OR": r = a | b
            elif name == "NOT": r = ~a
            else: r = np.where(a, b, args[2])
            stack.append(r)
    res = Result()
    res.is_mask, res.zero_tie = is_mask, tie
    out = stack[0]
    if is_mask:
        res.mask = np.asarray(out, dtype=bool)
        res.count = int(res.mask.sum())
        return res
    any_null = np.zeros(n, dtype=bool)
    for j in named:
        if cols[j][1] is not None:
            any_null |= np.asarray(cols[j][1], dtype=bool)[:n]
    values = np.ascontiguousarray(out, dtype=np.float64).copy()
    nan = np.isnan(values)
    values.view(np.uint64)[nan] = CANON_NAN
    res.values, res.nulls = values, nan & any_null
    res.count = int(res.nulls.sum())
    return res


def pack(flags):
    return np.packbits(np.asarray(flags, dtype=bool), bitorder="little")


RANDOM_SEED, RANDOM_PROGRAMS, RANDOM_ROWS = 2, 200, 5003      # the GPU test's random programs: no opposite-zero MAX / MIN among them


def three_columns(n, seed=1):
    """An F64 column, a masked I64 column and a masked BOOLBITS column of n rows."""
    rng = np.random.default_rng(seed)
    a = np.round(rng.normal(0.0, 50.0, n), 2)
    a[rng.random(n) < 0.05] = np.nan
    a[rng.random(n) < 0.02] = np.inf
    b = rng.integers(-1000, 1000, n)
    b[b == 0] = 7                                                           # no zero meets a -0.0 under MAX / MIN
    a[a == 0] = 0.25
    flag = rng.random(n) < 0.5
    return [(a, None, F64), (b.astype(np.int64), rng.random(n) < 0.1, I64), (flag, rng.random(n) < 0.1, BOOLBITS)]


def random_program(rng, dtypes, max_ops=MAX_OPS, max_depth=MAX_DEPTH, want_mask=None):
    """A random well-typed program over columns of the given dtypes: grows a typed stack with pushes and ops until the length
    budget is near, then folds it down to one entry (of the wanted type when want_mask is given)."""
    value_cols = [j for j, d in enumerate(dtypes) if d in (I64, F64)]
    bool_cols = [j for j, d in enumerate(dtypes) if d == BOOLBITS]
    consts = [0.5, -1.0, 2.0, 3.0, 1e-3, -7.25, 1e300, 0.1, 10.0]
    target = int(rng.integers(1, max_ops + 1))
    prog, stack = [], []

    def push():
        if bool_cols and rng.random() < 0.15:
            prog.append((OP["COL"], float(rng.choice(bool_cols))))
            stack.append(True)
        elif rng.random() < 0.7:
            prog.append((OP["COL"], float(rng.choice(value_cols))))
            stack.append(False)
        else:
            prog.append((OP["CONST"], float(rng.choice(consts))))
            stack.append(False)

    def fold():
        """One op over the top of the stack; False when none applies."""
        top = stack[-3:]
        cands = []
        if stack and not stack[-1]:
            cands += UNARY_VALUE + CLASSIFY
        if stack and stack[-1]:
            cands += [OP["NOT"]]
        if len(stack) >= 2 and not stack[-1] and not stack[-2]:
            cands += BINARY_VALUE * 2 + COMPARE
        if len(stack) >= 2 and stack[-1] and stack[-2]:
            cands += [OP["AND"], OP["OR"]] * 2
        if len(top) == 3 and top[0] and top[1] == top[2]:
            cands += [OP["SELECT"]] * 6
        if not cands:
            return False
        op = int(rng.choice(cands))
        pops = pops_of(op)
        out = stack[-1] if op == OP["SELECT"] else op in COMPARE or op in CLASSIFY or op in (OP["AND"], OP["OR"], OP["NOT"])
        del stack[len(stack) - pops:]
        stack.append(out)
        prog.append((op, 0.0))
        return True

    def reduce_one():
        """Shrinks the stack by one entry with the shortest fix-up: a binary op, after turning the top two into one type."""
        a, b = stack[-2], stack[-1]
        if a == b:
            op = int(rng.choice(BINARY_VALUE if not a else [OP["AND"], OP["OR"]]))
            prog.append((op, 0.0))
            stack.pop()
        elif b:                                             # value, boolean -> value: cond ? v : const needs cond first; compare instead
            prog.append((OP["NOT"], 0.0))                   # keep the boolean, then make the value under it a boolean too
            prog.append((OP["CONST"], 1.0)), stack.append(False)
            prog.append((OP["CONST"], 0.0)), stack.append(False)
            prog.append((OP["SELECT"], 0.0)), stack.pop(), stack.pop(), stack.pop(), stack.append(False)
            prog.append((OP["ADD"], 0.0)), stack.pop()
        else:                                               # boolean, value -> boolean
            prog.append((OP["ISNAN"], 0.0))
            stack[-1] = True
            prog.append((OP["OR"], 0.0)), stack.pop()

    while len(prog) + 6 * max(len(stack), 1) + 8 < target:
        if len(stack) < max_depth - 2 and (len(stack) < 2 or rng.random() < 0.45):
            push()
        elif not fold():
            push() if len(stack) < max_depth - 2 else reduce_one()
    if not stack:
        push()
    while len(stack) > 1:
        reduce_one()
    if want_mask is True and not stack[0]:
        prog.append((OP["CONST"], 0.0)), prog.append((OP["GT"], 0.0))
    if want_mask is False and stack[0]:
        prog.append((OP["CONST"], 1.0)), prog.append((OP["CONST"], -1.0)), prog.append((OP["SELECT"], 0.0))
        stack[0] = False
    elif want_mask is True:
        stack[0] = True
    while len(prog) < target:                               # the rest of the budget: ops that keep the one entry's type
        prog.append((int(rng.choice(UNARY_VALUE)) if not stack[0] else OP["NOT"], 0.0))
    return prog
