"""Thin host wrapper over the C ABI: one `Context` = one HIP stream + workspace on one GPU.

Columns are `(data, null_mask, dtype)` triples.  `data`/`null_mask` are either numpy arrays
(host memory: the library stages them over PCIe) or torch CUDA tensors (device memory: nothing
leaves HBM).  torch is used only as the device allocator; no torch op is on the compute path.
"""
import ctypes as C

import numpy as np

from . import _lib as L

_NP_OF = {L.I64: np.int64, L.F64: np.float64, L.U32CODE: np.uint32, L.BOOLBITS: np.uint8, L.CELL64: np.uint64}
# numpy dtype -> the torch dtype (by name: torch is imported lazily) that holds its bits on the device; unsigned 64- and
# 32-bit cells travel as the signed type of the same width
_TORCH_OF = {np.int64: "int64", np.uint64: "int64", np.float64: "float64", np.int32: "int32", np.uint32: "int32",
             np.uint8: "uint8"}


class PandrsHipError(RuntimeError):
    """Maps onto pandrs::Error (reference src/core/error.rs): .status is the C status code."""

    def __init__(self, status, message):
        super().__init__("[status %d] %s" % (status, message))
        self.status = status
        self.message = message


class ColumnTypeMismatch(PandrsHipError):
    pass


class OperationFailed(PandrsHipError):
    pass


class BelowThreshold(PandrsHipError):
    """PANDRS_HIP_ERR_BELOW_THRESHOLD: fewer rows than GpuConfig.min_size_threshold — the caller keeps its CPU path
    (src/optimized/split_dataframe/gpu.rs:30-32).  This package has no CPU path: the error is the answer."""


class EmptyError(PandrsHipError):
    """Error::Empty (src/optimized/split_dataframe/aggregate.rs:87): no non-null value to aggregate."""


def _raise(status):
    msg = L.last_error()
    if status == L.ERR_TYPE_MISMATCH:
        raise ColumnTypeMismatch(status, msg)
    if status == L.ERR_OPERATION_FAILED:
        raise OperationFailed(status, msg)
    if status == L.ERR_BELOW_THRESHOLD:
        raise BelowThreshold(status, msg)
    raise PandrsHipError(status, msg)


def _check(st):
    """Every C call returns a status; anything but 0 becomes the exception of its code."""
    if st:
        _raise(st)


def _is_torch(x):
    return x is not None and type(x).__module__.startswith("torch")


def _ptr(x):
    if x is None:
        return None
    if _is_torch(x):
        return x.data_ptr()
    return x.ctypes.data


def _space(on_device):
    return L.MEM_DEVICE if on_device else L.MEM_HOST


def _fill_bits(fill, dtype):
    """The 64-bit cell that stands for `fill`: the f64's bits for an F64 column, else the integer's low 64 bits."""
    return int(np.float64(fill).view(np.uint64)) if dtype == L.F64 else int(fill) & 0xFFFFFFFFFFFFFFFF


class ResidentColumn:
    """A column uploaded ONCE with `Context.upload_column` (pandrs_hip_column_upload): usable wherever a
    (data, null_mask, dtype) triple is, any number of times, until `release()` / the context is closed.  The
    reference's columns are immutable Arc<[T]> (src/column/int64_column.rs:10), so a shim can keep them in HBM
    across aggregate / join calls (src/optimized/dataframe/transformations.rs:524-577)."""

    def __init__(self, ctx, desc, n_rows):
        self.ctx, self.desc, self.n_rows, self.dtype = ctx, desc, n_rows, desc.dtype

    def release(self):
        if self.desc is not None and getattr(self.ctx, "h", None):
            st = self.ctx.lib.pandrs_hip_column_release(self.ctx.h, C.byref(self.desc))
            self.desc = None
            _check(st)
        self.desc = None

    def __iter__(self):        # unpacks like a triple: (self, None, dtype)
        return iter((self, None, self.dtype))

    def __getitem__(self, i):  # ... and indexes like one (col[0] is the data, col[2] the dtype)
        return (self, None, self.dtype)[i]

    def __len__(self):
        return 3


class Context:
    def __init__(self, device=0):
        self.lib = L.load()
        h = C.c_void_p()
        _check(self.lib.pandrs_hip_ctx_create(int(device), C.byref(h)))
        self.h = h
        self.device = device
        self.grouping_token = 0     # bumped by every groupby_indices: whose grouping the context retains (see grouped)

    def close(self):
        self.comm_destroy()
        if getattr(self, "h", None):
            self.lib.pandrs_hip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ---------------------------------------------------------------------------------
    def _cols(self, cols, keep, wait=True):
        arr = (L.Column * max(len(cols), 1))()
        space = None
        for i, (data, mask, dt) in enumerate(cols):
            if isinstance(data, ResidentColumn):
                if data.desc is None or data.ctx is not self:
                    raise ValueError("resident column released, or uploaded through another context")
                if space not in (None, L.MEM_DEVICE):
                    raise ValueError("columns of one call must all be host or all device")
                space = L.MEM_DEVICE
                keep.append(data)
                arr[i].data, arr[i].null_mask, arr[i].dtype = data.desc.data, data.desc.null_mask, data.desc.dtype
                continue
            if _is_torch(data):
                sp = L.MEM_DEVICE
                if not data.is_contiguous():
                    data = data.contiguous()
                if mask is not None and not _is_torch(mask):
                    raise ValueError("device column with a host null mask")
            else:
                sp = L.MEM_HOST
                data = np.ascontiguousarray(data, dtype=_NP_OF[dt])
                if mask is not None:
                    mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if space is None:
                space = sp
            elif space != sp:
                raise ValueError("columns of one call must all be host or all device")
            keep.extend([data, mask])
            arr[i].data = _ptr(data)
            arr[i].null_mask = _ptr(mask)
            arr[i].dtype = int(dt)
        if space == L.MEM_DEVICE and wait and any(_is_torch(next(iter(c))) for c in cols):
            self._wait_for_producer()
        return arr, (space if space is not None else L.MEM_HOST)

    def _col(self, col):
        """One column through _cols.  -> (Column array, memory space, keep): `keep` holds what the array's pointers point
        into, so the caller keeps it referenced until its C call has returned."""
        keep = []
        cc, sp = self._cols([tuple(col)], keep)
        return cc, sp, keep

    def _wait_for_producer(self):
        """The library runs on its own non-blocking stream and (like any C ABI over raw device
        pointers) requires its device inputs to be complete when the call starts.  Tensors handed
        over from torch may still be being written by kernels queued on torch's current stream."""
        import torch
        torch.cuda.current_stream(self.device).synchronize()

    @staticmethod
    def _aggs(aggs):
        arr = (L.AggSpec * max(len(aggs), 1))()
        for i, (c, op) in enumerate(aggs):
            arr[i].col, arr[i].op = int(c), int(op)
        return arr

    def _empty(self, shape, np_dtype, device):
        """Uninitialised storage for a result: a numpy array, or with `device` a torch tensor on this context's GPU."""
        if not device:
            return np.empty(shape, np_dtype)
        import torch
        return torch.empty(shape, dtype=getattr(torch, _TORCH_OF[np_dtype]), device="cuda:%d" % self.device)

    def _made(self, count, np_dtype, device):
        """A result buffer of the wrapper's own for `count` cells: exact on the host; on the device at least one cell,
        sliced to count."""
        if device:
            return self._empty(max(count, 1), np_dtype, True)[:count]
        return self._empty(count, np_dtype, False)

    def _given(self, out, count, np_dtype, what, name="out"):
        """Checks a caller's result buffer for `count` cells of `np_dtype` (`what` names the count in the error).
        -> whether it lives on the device."""
        device = _is_torch(out)
        if device:
            import torch
            ok = out.dtype == getattr(torch, _TORCH_OF[np_dtype]) and out.is_contiguous() and out.is_cuda and out.numel() >= count
        else:
            ok = isinstance(out, np.ndarray) and out.dtype == np_dtype and out.flags.c_contiguous and out.size >= count
        if not ok:
            raise ValueError("%s must be a contiguous %s numpy array or CUDA tensor of at least %s elements"
                             % (name, np.dtype(np_dtype).name, what))
        return device

    def _out_buffer(self, count, np_dtype, sp, out, out_device, what):
        """Where a call writes `count` cells of `np_dtype`.  -> (buffer of exactly count cells, lives on the device).
        A caller's `out` decides the space and comes back as a view of its first cells, once it has been checked and, for
        a CUDA tensor, torch's stream has been waited for.  Else out_device decides, else the space `sp` of the input."""
        if out is not None:
            out_device = self._given(out, count, np_dtype, what)
            if out_device:
                self._wait_for_producer()
            return out[:count], out_device
        if out_device is None:
            out_device = sp == L.MEM_DEVICE
        return self._made(count, np_dtype, out_device), out_device

    def _cell_outs(self, n, sp, want_i64, out, out_mask, out_device):
        """The (out, out_mask, out_device) a call with one 8-byte cell per row and a null bitmap writes into: as
        _out_buffer for each, but the two share one space and one wait, and both are checked before either is made."""
        cell, nbytes = (np.int64 if want_i64 else np.float64), (n + 7) // 8
        if out is not None or out_mask is not None:
            if out is not None and out_mask is not None and _is_torch(out) != _is_torch(out_mask):
                raise ValueError("out and out_mask must both be numpy arrays or both CUDA tensors")
            if out is not None:
                out_device = self._given(out, n, cell, "n_rows")
            if out_mask is not None:
                out_device = self._given(out_mask, nbytes, np.uint8, "ceil(n_rows / 8)", "out_mask")
            if out_device:
                self._wait_for_producer()
        elif out_device is None:
            out_device = sp == L.MEM_DEVICE
        out = self._made(n, cell, out_device) if out is None else out[:n]
        out_mask = self._made(nbytes, np.uint8, out_device) if out_mask is None else out_mask[:nbytes]
        return out, out_mask, out_device

    def _mask_out(self, n, sp, out, out_device, count_only):
        """The out_bits buffer of predicate / isin: -> (buffer or None, lives on the device)."""
        if count_only:
            if out is not None:
                raise ValueError("count_only takes no out")
            return None, False
        return self._out_buffer((n + 7) // 8, np.uint8, sp, out, out_device, "ceil(n_rows / 8)")

    def _code_rank(self, code_rank, sp, keep):
        """A string pool's rank table in the memory space `sp` of the call.  -> (table or None, n_codes)"""
        if code_rank is None:
            return None, 0
        if sp != L.MEM_DEVICE:
            rank = np.ascontiguousarray(code_rank.cpu().numpy() if _is_torch(code_rank) else code_rank).view(np.uint32)
        elif _is_torch(code_rank):
            rank = code_rank
            self._wait_for_producer()
        else:
            import torch
            rank = torch.from_numpy(np.ascontiguousarray(code_rank, dtype=np.uint32).view(np.int32)).to("cuda:%d" % self.device)
        keep.append(rank)
        return rank, int(rank.numel() if _is_torch(rank) else rank.shape[0])

    # -- resident columns -------------------------------------------------------------------------
    def upload_column(self, data, mask, dtype):
        """Host column -> HBM, once (pandrs_hip_column_upload).  -> ResidentColumn."""
        data = np.ascontiguousarray(data, dtype=_NP_OF[dtype])
        n = int(data.shape[0]) * (8 if dtype == L.BOOLBITS else 1)
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if dtype != L.BOOLBITS:
                assert mask.shape[0] >= (n + 7) // 8
        return self.upload_column_n(data, mask, dtype, n)

    def upload_column_n(self, data, mask, dtype, n_rows):
        host = L.Column(_ptr(data), _ptr(mask), int(dtype), 0)
        dev = L.Column()
        _check(self.lib.pandrs_hip_column_upload(self.h, C.byref(host), int(n_rows), C.byref(dev)))
        return ResidentColumn(self, dev, int(n_rows))

    def resident_bytes(self):
        b, n = C.c_int64(0), C.c_int64(0)
        _check(self.lib.pandrs_hip_resident_bytes(self.h, C.byref(b), C.byref(n)))
        return b.value, n.value

    def synchronize(self):
        _check(self.lib.pandrs_hip_ctx_synchronize(self.h))

    def set_option(self, name, value):
        _check(self.lib.pandrs_hip_ctx_set_option(self.h, name.encode(), int(value)))

    def reserve(self, nbytes):
        _check(self.lib.pandrs_hip_ctx_reserve(self.h, int(nbytes)))

    def timings(self):
        t = L.Timings()
        _check(self.lib.pandrs_hip_get_timings(self.h, C.byref(t)))
        return {
            "total_ms": t.total_ms,
            "phase_ms": {L.PHASE_NAMES[i]: t.phase_ms[i] for i in range(L.MAX_PHASES)
                         if L.PHASE_NAMES[i] and t.phase_ms[i] > 0},
            "algorithmic_bytes": t.algorithmic_bytes, "n_partitions": t.n_partitions,
            "table_slots": t.table_slots, "retries": t.retries,
            "estimated_groups": t.estimated_groups, "absorbed_rows": t.absorbed_rows,
        }

    # -- groupby -----------------------------------------------------------------------------------
    def groupby_compute(self, keys, n_rows, vals, aggs):
        """Runs the device pipeline and keeps the result in the context.  -> n_groups."""
        keep = []
        kc, sp1 = self._cols(keys, keep, wait=not vals)       # one wait covers both column lists
        vc, sp2 = self._cols(vals, keep) if vals else ((L.Column * 1)(), sp1)
        if vals and sp1 != sp2:
            raise ValueError("keys and values must live in the same memory space")
        ng = C.c_int64(0)
        _check(self.lib.pandrs_hip_groupby_agg(self.h, sp1, kc, len(keys), int(n_rows), vc, len(vals),
                                               self._aggs(aggs), len(aggs), C.byref(ng)))
        self._last = (len(keys), len(aggs), sp1, ng.value)
        return ng.value

    def groupby_fetch(self, to_device=None):
        """-> (key_cells[n_keys, G] u64, key_null[n_keys, G] u8, aggs[n_aggs, G] f64)."""
        n_keys, n_aggs, space, g = self._last
        dev = space == L.MEM_DEVICE if to_device is None else to_device
        kc = self._empty((n_keys, g), np.uint64, dev)
        kn = self._empty((n_keys, g), np.uint8, dev)
        oa = self._empty((n_aggs, g), np.float64, dev)
        pk = (C.c_void_p * max(n_keys, 1))(*[_ptr(kc[i]) for i in range(n_keys)])
        pn = (C.c_void_p * max(n_keys, 1))(*[_ptr(kn[i]) for i in range(n_keys)])
        pa = (C.c_void_p * max(n_aggs, 1))(*[_ptr(oa[i]) for i in range(n_aggs)])
        _check(self.lib.pandrs_hip_groupby_fetch(self.h, _space(dev), pk, pn, pa))
        return kc, kn, oa

    def groupby_agg(self, keys, n_rows, vals, aggs):
        self.groupby_compute(keys, n_rows, vals, aggs)
        return self.groupby_fetch()

    def groupby_indices_compute(self, keys, n_rows):
        """The grouping alone: it stays in the context for groupby_indices' fetch and for any number of grouped() calls.
        -> (n_groups, memory space of the keys).  Bumps grouping_token: a caller that remembers the value it saw after its
        own call knows later whether the retained grouping is still its own."""
        keep = []
        kc, sp = self._cols(keys, keep)
        ng = C.c_int64(0)
        self.grouping_token += 1                        # (a failed call drops the retained grouping too)
        _check(self.lib.pandrs_hip_groupby_indices(self.h, sp, kc, len(keys), int(n_rows), C.byref(ng)))
        return ng.value, sp

    def groupby_indices(self, keys, n_rows):
        """group_by's row -> group assignment (grouping.rs:22-115) in CSR form.
        -> (key_cells[n_keys, G] u64, key_null[n_keys, G] u8, offsets[G + 1] i64, rows[n_rows] i64);
        group g = rows[offsets[g]:offsets[g + 1]], ascending."""
        g, sp = self.groupby_indices_compute(keys, n_rows)
        nk, dev = len(keys), sp == L.MEM_DEVICE
        cells = self._empty((nk, g), np.uint64, dev)
        nulls = self._empty((nk, g), np.uint8, dev)
        off = self._empty(g + 1, np.int64, dev)
        rows = self._empty(int(n_rows), np.int64, dev)
        pk = (C.c_void_p * nk)(*[_ptr(cells[i]) for i in range(nk)])
        pn = (C.c_void_p * nk)(*[_ptr(nulls[i]) for i in range(nk)])
        _check(self.lib.pandrs_hip_groupby_indices_fetch(self.h, sp, pk, pn, _ptr(off), _ptr(rows)))
        return cells, nulls, off, rows

    def groupby_agg_chunked(self, keys, n_rows, vals, aggs, chunk_rows):
        """Groupby over more rows than one call takes (the per-call limit is 2^32 rows: 32-bit row
        offsets) or than the workspace should hold at once: the rows are processed in chunks of
        `chunk_rows` (a multiple of 8, so that null bitmaps split on byte boundaries), every chunk
        leaves mergeable partial states, and one merge finishes.  Single key column and the mergeable
        aggregates (Sum / Mean / Min / Max / Count), like the multi-GPU path it reuses."""
        if chunk_rows <= 0 or chunk_rows % 8:
            raise ValueError("chunk_rows must be a positive multiple of 8")
        if len(keys) != 1:
            raise NotImplementedError("chunked groupby takes one key column")
        def cut(col, lo, hi):
            data, mask, dt = col
            if dt == L.BOOLBITS:
                data = data[lo // 8:(hi + 7) // 8]
            else:
                data = data[lo:hi]
            return (data, None if mask is None else mask[lo // 8:(hi + 7) // 8], dt)
        recs = []
        for lo in range(0, int(n_rows), int(chunk_rows)):
            hi = min(lo + int(chunk_rows), int(n_rows))
            self.groupby_partials([cut(keys[0], lo, hi)], hi - lo, [cut(v, lo, hi) for v in vals], aggs)
            rec, _ = self.partials_split(1)
            recs.append(rec)
        if not recs:
            return self.groupby_agg(keys, 0, vals, aggs)
        if _is_torch(recs[0]):
            import torch
            allrec = torch.cat(recs, dim=0)
        else:
            allrec = np.concatenate(recs, axis=0)
        self.groupby_merge(keys[0][2], allrec, [v[2] for v in vals], [v[1] is not None for v in vals], aggs)
        return self.groupby_fetch()

    # -- row shuffle by key owner (multi-GPU) ------------------------------------------------------------
    def shuffle_split(self, key, payload, n_rows, n_ranks, drop_null_keys=False):
        """Buckets this shard's rows by the owner rank of their key, rank-contiguous.
        -> (cells[n] u64, key_null[n] u8, [payload u64/i64 [n]], [payload null bytes [n] or None], counts[n_ranks])"""
        keep = []
        kc, sp = self._cols([key], keep)
        pc, sp2 = self._cols(payload, keep) if payload else ((L.Column * 1)(), sp)
        if payload and sp != sp2:
            raise ValueError("key and payload must live in the same memory space")
        counts = (C.c_int64 * n_ranks)()
        n_out = C.c_int64(0)
        _check(self.lib.pandrs_hip_shuffle_split(self.h, sp, kc, pc, len(payload), int(n_rows), int(n_ranks),
                                                 1 if drop_null_keys else 0, counts, C.byref(n_out)))
        n, npay, dev = n_out.value, len(payload), sp == L.MEM_DEVICE
        cells, knull = self._empty(n, np.uint64, dev), self._empty(n, np.uint8, dev)
        pays = [self._empty(n, np.uint64, dev) for _ in range(npay)]
        pnull = [self._empty(n, np.uint8, dev) if p[1] is not None else None for p in payload]
        pp = (C.c_void_p * max(npay, 1))(*[_ptr(a) for a in pays])
        pn = (C.c_void_p * max(npay, 1))(*[_ptr(a) for a in pnull])
        _check(self.lib.pandrs_hip_shuffle_fetch(self.h, sp, _ptr(cells), _ptr(knull), pp, pn))
        return cells, knull, pays, pnull, [int(x) for x in counts]

    def key_hash_cells(self, keys, n_rows):
        """One 64-bit hash cell per row of a composite key (the shuffle key of a multi-key groupby)."""
        keep = []
        kc, sp = self._cols(keys, keep)
        out = self._empty(int(n_rows), np.uint64, sp == L.MEM_DEVICE)
        _check(self.lib.pandrs_hip_key_hash_cells(self.h, sp, kc, len(keys), int(n_rows), _ptr(out)))
        return out

    def bytes_to_bitmap(self, flags):
        """One byte per row (non-zero = set) -> LSB-first bitmap, same kind (numpy / torch) as the input."""
        n = int(flags.shape[0])
        dev = _is_torch(flags)
        if dev:
            self._wait_for_producer()
            flags = flags.contiguous()
        else:
            flags = np.ascontiguousarray(flags, np.uint8)
        out = self._empty((n + 7) // 8, np.uint8, dev)
        _check(self.lib.pandrs_hip_bytes_to_bitmap(self.h, _space(dev), _ptr(flags), n, _ptr(out)))
        return out

    # -- mergeable partials (multi-GPU) --------------------------------------------------------------
    def groupby_partials(self, keys, n_rows, vals, aggs):
        """-> (n_groups, n_state); partial rows stay in the context until partials_split."""
        keep = []
        kc, sp1 = self._cols(keys, keep)
        vc, _ = self._cols(vals, keep) if vals else ((L.Column * 1)(), sp1)
        ng, ns = C.c_int64(0), C.c_int32(0)
        _check(self.lib.pandrs_hip_groupby_partials(self.h, sp1, kc, len(keys), int(n_rows), vc, len(vals),
                                                    self._aggs(aggs), len(aggs), C.byref(ng), C.byref(ns)))
        self._last_partials = (ng.value, ns.value, sp1)
        return ng.value, ns.value

    def partials_split(self, n_ranks, device=None):
        """Buckets the retained partial rows by owner rank.
        -> (records[G, 2 + n_state] int64/uint64: key, key_null, states..., counts[n_ranks]);
        records are rank-contiguous, ready for one all-to-all."""
        g, ns, space = self._last_partials
        dev = space == L.MEM_DEVICE if device is None else device
        counts = (C.c_int64 * n_ranks)()
        rec = self._empty((g, 2 + ns), np.uint64, dev)
        _check(self.lib.pandrs_hip_partials_split(self.h, _space(dev), n_ranks, _ptr(rec), counts))
        return rec, [int(c) for c in counts]

    def groupby_merge(self, key_dtype, records, val_dtypes, val_has_nulls, aggs):
        """records: [n, 2 + n_state] packed partial rows gathered from all peers."""
        dev = _is_torch(records)
        if not dev:
            records = np.ascontiguousarray(records, np.uint64)
        else:
            records = records.contiguous()
            self._wait_for_producer()
        n_rows = int(records.shape[0])
        nv = len(val_dtypes)
        vd = (C.c_int32 * max(nv, 1))(*[int(x) for x in val_dtypes])
        vh = (C.c_uint8 * max(nv, 1))(*[1 if x else 0 for x in val_has_nulls])
        ng = C.c_int64(0)
        _check(self.lib.pandrs_hip_groupby_merge(self.h, _space(dev), int(key_dtype), _ptr(records) if n_rows else None, n_rows,
                                                 vd, nv, vh, self._aggs(aggs), len(aggs), C.byref(ng)))
        self._last = (1, len(aggs), _space(dev), ng.value)
        return ng.value

    # -- join --------------------------------------------------------------------------------------------
    def join_indices_compute(self, lkey, n_left, rkey, n_right, how):
        """Runs the join and keeps the pairs in the context (pandrs_hip_join_indices).  -> (n_pairs, memory space)"""
        keep = []
        lc, sp1 = self._cols([lkey], keep)
        rc, sp2 = self._cols([rkey], keep)
        if sp1 != sp2:
            raise ValueError("both key columns must live in the same memory space")
        n = C.c_int64(0)
        _check(self.lib.pandrs_hip_join_indices(self.h, sp1, lc, int(n_left), rc, int(n_right), int(how), C.byref(n)))
        return n.value, sp1

    def join_indices(self, lkey, n_left, rkey, n_right, how):
        n, sp1 = self.join_indices_compute(lkey, n_left, rkey, n_right, how)
        li, ri = self._empty(n, np.int64, sp1 == L.MEM_DEVICE), self._empty(n, np.int64, sp1 == L.MEM_DEVICE)
        _check(self.lib.pandrs_hip_join_fetch(self.h, sp1, _ptr(li), _ptr(ri)))
        return li, ri

    def gather(self, src, mask, idx, fill, dtype):
        """Device tensors only.  -> torch tensor (uint8 per row for BOOLBITS sources)."""
        self._wait_for_producer()        # src / mask / idx may still be being written on torch's current stream
        n = idx.numel()
        fn = {L.I64: self.lib.pandrs_hip_gather_i64, L.F64: self.lib.pandrs_hip_gather_f64,
              L.U32CODE: self.lib.pandrs_hip_gather_u32, L.BOOLBITS: self.lib.pandrs_hip_gather_bool}[dtype]
        out = self._empty(n, _NP_OF[dtype], True)
        fill = float(fill) if dtype == L.F64 else int(fill)
        _check(fn(self.h, L.MEM_DEVICE, _ptr(src), _ptr(mask), _ptr(idx), n, fill, _ptr(out)))
        return out

    def join_gather(self, col, n_src, n_out, side, fill=0, key_right=None, n_right=0):
        """One column of the joined frame through the pairs this context retains (the last join_indices / join_indices_compute):
        pandrs_hip_join_gather (side 0 = the pairs' left rows, 1 = their right rows), or — key_right given — pandrs_hip_join_gather_key
        (the left key's value, else the right key's: join.rs:364-470).  `col` is a (data, mask, dtype) triple on the host or the
        device, or a ResidentColumn; -> numpy array of n_out elements (uint8 per row for BOOLBITS sources)."""
        cc, sp, keep = self._col(col)
        dtype = tuple(col)[2]
        out = np.empty(int(n_out), {L.I64: np.int64, L.F64: np.float64, L.U32CODE: np.uint32, L.BOOLBITS: np.uint8}[dtype])
        if key_right is None:
            _check(self.lib.pandrs_hip_join_gather(self.h, sp, cc, int(n_src), int(side), _fill_bits(fill, dtype), L.MEM_HOST, _ptr(out)))
        else:
            kc, sp2 = self._cols([tuple(key_right)], keep)
            if sp2 != sp:
                raise ValueError("both key columns must live in one memory space")
            _check(self.lib.pandrs_hip_join_gather_key(self.h, sp, cc, int(n_src), kc, int(n_right), _fill_bits(fill, dtype),
                                                       L.MEM_HOST, _ptr(out)))
        return out

    def _join_groupby_sum(self, call, head, lkey, lval, n_left, rkey, rgroup, n_right):
        """call(*head, space, left key, left value, n_left, right key, right group, n_right, &n_groups), then the fetch."""
        keep = []
        (a, sp), (b, _), (c, _), (d, _) = [self._cols([x], keep) for x in (lkey, lval, rkey, rgroup)]
        ng = C.c_int64(0)
        _check(call(*head, sp, a, b, int(n_left), c, d, int(n_right), C.byref(ng)))
        self._last = (1, 1, sp, ng.value)
        return self.groupby_fetch()

    def join_groupby_sum(self, lkey, lval, n_left, rkey, rgroup, n_right):
        return self._join_groupby_sum(self.lib.pandrs_hip_join_groupby_sum, (self.h,), lkey, lval, n_left, rkey, rgroup, n_right)

    def column_std(self, col, n, population=True):
        """parallel_std_f64_value / parallel_var (jit/parallel.rs:222-250): sqrt(max(sum_sq / n - mean^2, 0)),
        n <= 1 => 0.0.  -> (std, variance)."""
        cc, sp, keep = self._col(col)
        s, q, cnt = C.c_double(0), C.c_double(0), C.c_int64(0)
        _check(self.lib.pandrs_hip_reduce_moments(self.h, sp, cc, int(n), C.byref(s), C.byref(q), C.byref(cnt)))
        m = cnt.value
        if m <= 1:
            return 0.0, 0.0
        mean = s.value / m
        var = max(q.value / m - mean * mean, 0.0)
        if not population:
            var *= m / (m - 1.0)
        return var ** 0.5, var

    # -- the in-library RCCL exchange (pandrs_hip_dist_*) -------------------------------------------------
    @staticmethod
    def comm_unique_id():
        """128 bytes from rank 0 (ncclGetUniqueId); the host hands them to every rank over any channel."""
        buf = C.create_string_buffer(128)
        _check(L.load().pandrs_hip_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        h = C.c_void_p()
        _check(self.lib.pandrs_hip_comm_init(self.h, C.c_char_p(bytes(unique_id)), int(rank), int(world), C.byref(h)))
        self.comm = h
        self.comm_world = world
        return h

    def comm_adopt_transport(self, all_gather, all_reduce_max, all_to_all_v, rank, world):
        """pandrs_hip_comm_adopt_transport: the in-library exchange over host callbacks instead of RCCL.
        all_gather(send: bytes) -> list of world bytes objects; all_reduce_max(list of int) -> list of int;
        all_to_all_v(list of world bytes objects) -> list of world bytes objects (what each rank sent to this one)."""
        def _ag(_user, send, recv, nbytes):
            try:
                parts = all_gather(C.string_at(send, nbytes))
                for r, part in enumerate(parts):
                    assert len(part) == nbytes
                    C.memmove(recv + r * nbytes, part, nbytes)
                return 0
            except Exception:        # noqa: BLE001 — the library turns a non-zero status into an error on every rank
                import traceback
                traceback.print_exc()
                return 1

        def _ar(_user, vals, n):
            try:
                out = all_reduce_max([int(vals[i]) for i in range(n)])
                for i in range(n):
                    vals[i] = int(out[i])
                return 0
            except Exception:        # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1

        def _a2a(_user, send, sb, so, recv, rb, ro):
            try:
                parts = all_to_all_v([C.string_at(send + so[p], sb[p]) if sb[p] else b"" for p in range(world)])
                for p in range(world):
                    assert len(parts[p]) == rb[p], (p, len(parts[p]), rb[p])
                    if rb[p]:
                        C.memmove(recv + ro[p], parts[p], rb[p])
                return 0
            except Exception:        # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1

        t = L.Transport(None, L.ALL_GATHER_FN(_ag), L.ALL_REDUCE_MAX_FN(_ar), L.ALL_TO_ALL_V_FN(_a2a))
        h = C.c_void_p()
        _check(self.lib.pandrs_hip_comm_adopt_transport(C.byref(t), int(rank), int(world), C.byref(h)))
        self._transport = t            # the callbacks must outlive the communicator
        self.comm = h
        self.comm_world = world
        return h

    @staticmethod
    def alloc_events():
        n = C.c_int64(0)
        L.load().pandrs_hip_alloc_events(C.byref(n))
        return n.value

    @staticmethod
    def workspace_poisoned_bytes():
        """Bytes of workspace the "poison_workspace" knob has filled since the library was loaded."""
        n = C.c_int64(0)
        L.load().pandrs_hip_workspace_poisoned_bytes(C.byref(n))
        return n.value

    @staticmethod
    def poison_workspace(byte):
        """Testing knob (process-wide): fill every workspace block with `byte` (0 ... 255) before a call uses it; None = off."""
        value = 0 if byte is None else (int(byte) & 0xFF) or 0x100
        _check(L.load().pandrs_hip_ctx_set_option(None, b"poison_workspace", value))

    def comm_destroy(self):
        if getattr(self, "comm", None):
            self.lib.pandrs_hip_comm_destroy(self.comm)
            self.comm = None

    def dist_groupby_compute(self, keys, n_rows, vals, aggs):
        """pandrs_hip_dist_groupby_agg: every rank passes its own row range.  -> groups owned by this rank."""
        keep = []
        kc, sp1 = self._cols(keys, keep)
        vc, _ = self._cols(vals, keep) if vals else ((L.Column * 1)(), sp1)
        ng = C.c_int64(0)
        _check(self.lib.pandrs_hip_dist_groupby_agg(self.h, self.comm, sp1, kc, len(keys), int(n_rows), vc, len(vals),
                                                    self._aggs(aggs), len(aggs), C.byref(ng)))
        general = len(keys) > 1 or any(int(op) > L.COUNT for _, op in aggs)
        self._last = (len(keys), len(aggs), L.MEM_DEVICE if general else sp1, ng.value)     # the row shuffle leaves its result on the device
        return ng.value

    def dist_join_groupby_sum(self, lkey, lval, n_left, rkey, rgroup, n_right):
        return self._join_groupby_sum(self.lib.pandrs_hip_dist_join_groupby_sum, (self.h, self.comm), lkey, lval, n_left, rkey, rgroup,
                                      n_right)

    def column_stats(self, col, n):
        """pandrs_hip_reduce_stats: one pass, everything K1's reference functions need.  -> dict."""
        cc, sp, keep = self._col(col)
        out = L.ColumnStats()
        _check(self.lib.pandrs_hip_reduce_stats(self.h, sp, cc, int(n), C.byref(out)))
        return {name: getattr(out, name) for name, _ in L.ColumnStats._fields_}

    def reduce_column(self, col, n):
        cc, sp, keep = self._col(col)
        out = (C.c_double * 4)()
        cnt = C.c_int64(0)
        _check(self.lib.pandrs_hip_reduce_column(self.h, sp, cc, int(n), out, C.byref(cnt)))
        return np.array(list(out)), cnt.value

    # -- sort ----------------------------------------------------------------------------------------------
    def sort_indices(self, keys, n_rows, ascending=None, code_rank=None):
        """OptimizedDataFrame::sort_by_columns' row order (split_dataframe/sort.rs:18-272) on the device
        (pandrs_hip_sort_indices): the stable permutation ordering the rows by keys[0], then keys[1], ...; nulls last
        in both directions, NaN after every number and before nulls.  `keys` are (data, null_mask, dtype) triples
        (host, device or ResidentColumn), `ascending` one flag per key (None = all ascending), `code_rank` the string
        pool's rank table (rank[code] = position of the code's string in byte-wise order), needed when a key is a
        string column.  -> int64 torch tensor of n_rows row indices on this context's device."""
        keep = []
        kc, sp = self._cols(keys, keep)
        nk = len(keys)
        asc = None
        if ascending is not None:
            asc = (C.c_int32 * max(nk, 1))(*[1 if a else 0 for a in ascending])
        rank, n_codes = self._code_rank(code_rank, sp, keep)
        out = self._empty(int(n_rows), np.int64, True)
        _check(self.lib.pandrs_hip_sort_indices(self.h, sp, kc, nk, asc, _ptr(rank), n_codes, int(n_rows), L.MEM_DEVICE,
                                                _ptr(out) if n_rows else None))
        return out

    # -- filter (stream compaction) ---------------------------------------------------------------------------
    def filter_indices(self, cond, n_rows, indices=True):
        """OptimizedDataFrame::filter's selection (split_dataframe/data_ops.rs:37-121) on the device
        (pandrs_hip_filter_indices): the rows whose BOOLBITS condition is Some(true), ascending.  `cond` is a
        (bits, null_mask, dtype) triple (host, device or ResidentColumn).  The context keeps the selection for
        filter_gather until the next filter_indices.  -> (int64 torch tensor of the selected rows on this context's
        device, or None when indices=False, selected row count)."""
        cc, sp, keep = self._col(cond)
        out = self._empty(max(int(n_rows), 1), np.int64, True) if indices else None
        cnt = C.c_int64(0)
        _check(self.lib.pandrs_hip_filter_indices(self.h, sp, cc, int(n_rows), L.MEM_DEVICE, _ptr(out), C.byref(cnt)))
        return (out[:cnt.value] if indices else None), cnt.value

    def filter_gather(self, col, n_src, n_out, fill=0, out_device=False):
        """One column compacted through the selection of the last filter_indices (pandrs_hip_filter_gather): the
        selected rows' values in row order, nulls as `fill`, no mask.  `col` is a (data, mask, dtype) triple on the
        host or the device, or a ResidentColumn; n_out = the selection's count.  -> numpy array of n_out elements
        (uint8 per row for BOOLBITS sources), or with out_device a torch tensor on this context's device (int32 for
        U32CODE)."""
        cc, sp, keep = self._col(col)
        dtype = tuple(col)[2]
        np_dtype = {L.F64: np.float64, L.U32CODE: np.uint32, L.BOOLBITS: np.uint8}.get(dtype, np.int64)
        out, out_device = self._out_buffer(int(n_out), np_dtype, sp, None, bool(out_device), "n_out")
        _check(self.lib.pandrs_hip_filter_gather(self.h, sp, cc, int(n_src), _fill_bits(fill, dtype), _space(out_device),
                                                 _ptr(out) if int(n_out) else None))
        return out

    # -- window statistics (rolling / expanding / EWM) ----------------------------------------------------------
    def window(self, col, n_rows, kind, op, window=0, min_periods=-1, center=False, ddof=1, alpha=0.0, out_device=None):
        """One window statistic of one I64 / F64 column on the device (pandrs_hip_window; DataFrameWindowExt,
        src/dataframe/window.rs:13-160 over src/series/window.rs).  `col` is a (data, mask, dtype) triple on the host
        or the device, or a ResidentColumn; kind / op are L.WINDOW_KIND_* / L.WINDOW_*; window, min_periods (< 0 =
        window), center and ddof as the rolling spec, alpha resolved by the caller (EWM).  -> n_rows float64 values,
        NaN for None: a torch tensor on this context's device for device / resident columns (or out_device=True),
        else a numpy array."""
        cc, sp, keep = self._col(col)
        n = int(n_rows)
        spec = L.WindowSpec(kind=int(kind), op=int(op), window=int(window), min_periods=int(min_periods),
                            center=1 if center else 0, reserved=0, ddof=int(ddof), alpha=float(alpha))
        out, out_device = self._out_buffer(n, np.float64, sp, None, out_device, "n_rows")
        _check(self.lib.pandrs_hip_window(self.h, sp, cc, n, C.byref(spec), _space(out_device), _ptr(out) if n else None))
        return out

    def window_quantile(self, col, n_rows, kind, *, median=True, q=0.5, window=0, min_periods=-1, center=False, nan_missing=False,
                        out_device=None):
        """The rolling / expanding median (median=True) or quantile(q) of one I64 / F64 column on the device
        (pandrs_hip_window_quantile; Rolling / Expanding::{median, quantile}, src/series/window.rs:298-336, :494-530, and
        PandasCompatExt::rolling_median, helpers/window_ops.rs:206-240).  `col`, kind (L.WINDOW_KIND_ROLLING / _EXPANDING),
        window, min_periods (< 0 = window) and center as in window(); nan_missing=True also skips NaN cells
        (window_ops.rs:221).  A window with fewer than min_periods values, or none, gives NaN, as does (without
        nan_missing) one that holds a NaN value.  Same return conventions as window()."""
        cc, sp, keep = self._col(col)
        n = int(n_rows)
        spec = L.WindowQuantileSpec(kind=int(kind), median=1 if median else 0, window=int(window), min_periods=int(min_periods),
                                    center=1 if center else 0, nan_missing=1 if nan_missing else 0, q=float(q))
        out, out_device = self._out_buffer(n, np.float64, sp, None, out_device, "n_rows")
        _check(self.lib.pandrs_hip_window_quantile(self.h, sp, cc, n, C.byref(spec), _space(out_device), _ptr(out) if n else None))
        return out

    # -- describe / exact percentiles (radix select) -------------------------------------------------------------
    def describe(self, col, n_rows):
        """count, mean, std, min, 25%, 50%, 75%, max of one I64 / F64 column on the device (pandrs_hip_describe;
        OptimizedDataFrame::describe, split_dataframe/stats.rs:50-151 over stats/descriptive.rs:91-200).  `col` is a
        (data, mask, dtype) triple on the host or the device, or a ResidentColumn.  -> dict with the fields of
        pandrs_hip_describe_stats (count, mean, std, min, q1, median, q3, max); count 0 gives NaN everywhere."""
        cc, sp, keep = self._col(col)
        out = L.DescribeStats()
        _check(self.lib.pandrs_hip_describe(self.h, sp, cc, int(n_rows), C.byref(out)))
        return {name: getattr(out, name) for name, _ in L.DescribeStats._fields_}

    def quantiles(self, col, n_rows, percentiles):
        """percentile(sorted non-null values, p) (stats/descriptive.rs:169-200) for 1 to 16 values of p in [0, 100], in any
        order, on the device (pandrs_hip_quantiles).  `col` as in describe.  -> (float64 numpy array, one value per p,
        NaN when the column has no non-null cell; the non-null count)."""
        cc, sp, keep = self._col(col)
        ps = np.ascontiguousarray(percentiles, dtype=np.float64).reshape(-1)
        out = np.empty(max(ps.shape[0], 1), np.float64)
        cnt = C.c_int64(0)
        _check(self.lib.pandrs_hip_quantiles(self.h, sp, cc, int(n_rows), ps.ctypes.data_as(C.POINTER(C.c_double)), int(ps.shape[0]),
                                             out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cnt)))
        return out[:ps.shape[0]], cnt.value

    # -- shape statistics (fused sums of many columns; order statistics by the reference's index rules) -----------------
    def moments(self, cols, n_rows, want=0):
        """The fused sums of 1 to L.MOMENTS_MAX_COLUMNS I64 / F64 columns of n_rows rows each, in the same launches
        (pandrs_hip_moments; the sums behind PandasCompatExt::skew / kurtosis / sem / mad / prod / cv / geometric_mean /
        harmonic_mean / var_column / range / abs_sum / zscore and the *_all lists).  `cols`: (data, mask, dtype) triples, all
        on the host or all on the device, or ResidentColumns.  `want`: L.MOMENTS_WANT_CENTRAL | _LOG | _RECIP | _PROD; a
        field whose bit is clear is NaN.  Cells that are null or NaN do not count.  -> a list of dicts, one per column, with
        the fields of pandrs_hip_moments_stats."""
        cols = [tuple(c) for c in cols]
        keep = []
        cc, sp = self._cols(cols, keep)
        out = (L.MomentsStats * max(len(cols), 1))()
        _check(self.lib.pandrs_hip_moments(self.h, sp, cc, len(cols), int(n_rows), int(want), out))
        return [{name: getattr(out[i], name) for name, _ in L.MomentsStats._fields_} for i in range(len(cols))]

    def order_stats(self, col, n_rows, ops):
        """Order statistics of one I64 / F64 column by the reference's index rules, and the trimmed mean, on the device
        (pandrs_hip_order_stats; PandasCompatExt::iqr / describe_column / percentile_value / trimmed_mean / median_all).
        `col` as in describe; `ops`: 1 to L.ORDER_STATS_MAX_OPS pairs (op, arg) with op L.OS_AT_FRAC_N / _AT_FRAC_N1 /
        _MEDIAN / _TRIMMED_MEAN.  -> (float64 numpy array, one value per pair; m, the cells that are neither null nor NaN)."""
        cc, sp, keep = self._col(col)
        ops = list(ops)
        k = len(ops)
        op = np.ascontiguousarray([int(o) for o, _ in ops], dtype=np.int32).reshape(-1)
        arg = np.ascontiguousarray([float(a) for _, a in ops], dtype=np.float64).reshape(-1)
        out = np.empty(max(k, 1), np.float64)
        cnt = C.c_int64(0)
        _check(self.lib.pandrs_hip_order_stats(self.h, sp, cc, int(n_rows), op.ctypes.data_as(C.POINTER(C.c_int32)),
                                               arg.ctypes.data_as(C.POINTER(C.c_double)), k,
                                               out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cnt)))
        return out[:k], cnt.value

    # -- rank (radix sort, tie-run boundaries, scatter) ------------------------------------------------------------
    def rank(self, col, n_rows, method, out=None, out_device=None):
        """The ascending 1-based rank of every row of one I64 / F64 column on the device (pandrs_hip_rank;
        PandasCompatExt::rank, src/dataframe/pandas_compat/functions.rs:193-236).  `col` is a (data, mask, dtype) triple on
        the host or the device, or a ResidentColumn; method is L.RANK_AVERAGE / MIN / MAX / FIRST / DENSE.  NaN and null
        cells get NaN and take no rank.  `out`: a float64 numpy array or torch CUDA tensor of at least n_rows elements to
        write into.  -> n_rows float64 ranks: `out` when given; else a torch tensor on this context's device for device /
        resident columns (or out_device=True), else a numpy array."""
        cc, sp, keep = self._col(col)
        n = int(n_rows)
        out, out_device = self._out_buffer(n, np.float64, sp, out, out_device, "n_rows")
        _check(self.lib.pandrs_hip_rank(self.h, sp, cc, n, int(method), _space(out_device), _ptr(out) if n else None))
        return out

    # -- fill (valid bits, a carry across tiles, a nearby gather) ------------------------------------------------------
    def fill(self, col, n_rows, method, value=None, out=None, out_mask=None, out_device=None):
        """Missing cells of one I64 / F64 column repaired on the device (pandrs_hip_fill; PandasCompatExt::fillna /
        fillna_method / interpolate / ffill / bfill, src/dataframe/pandas_compat/functions.rs:789-918, :3626-3683).  A cell is
        missing when its null bit is set or, for F64, when it is NaN.  `col` is a (data, mask, dtype) triple on the host or
        the device, or a ResidentColumn; method is L.FILL_FFILL / BFILL / LINEAR / VALUE.  `value` (VALUE only): an int that
        fits int64 for an I64 column, a float for F64 (NaN leaves the rows missing).  `out` / `out_mask`: a numpy array or
        torch CUDA tensor (both in the same space) of at least n_rows cells of the result's dtype / ceil(n_rows / 8) uint8
        to write into.  -> (values, mask, n_missing): values is int64, or float64 for an F64 column and under LINEAR; mask
        is the uint8 null bitmap of the rows still missing, None when n_missing == 0.  Both are `out` / `out_mask` when
        given; else torch tensors on this context's device for device / resident columns (or out_device=True), else
        numpy arrays."""
        cc, sp, keep = self._col(col)
        n, method = int(n_rows), int(method)
        is_i64 = cc[0].dtype == L.I64
        fill_bits = 0
        if method == L.FILL_VALUE:
            if is_i64:
                if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not -(1 << 63) <= int(value) < (1 << 63):
                    raise ValueError("an I64 column is filled with an int that fits int64, got %r" % (value,))
            elif isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
                raise ValueError("an F64 column is filled with a float, got %r" % (value,))
            fill_bits = _fill_bits(value, L.I64 if is_i64 else L.F64)
        elif value is not None:
            raise ValueError("value goes with FILL_VALUE only")
        out, out_mask, out_device = self._cell_outs(n, sp, is_i64 and method != L.FILL_LINEAR, out, out_mask, out_device)
        missing = C.c_int64(0)
        _check(self.lib.pandrs_hip_fill(self.h, sp, cc, n, method, C.c_uint64(fill_bits), _space(out_device),
                                        _ptr(out) if n else None, _ptr(out_mask) if n else None, C.byref(missing)))
        return out, (out_mask if missing.value else None), missing.value

    # -- cumulative folds and lags (reduce then apply over spans; one stream) -----------------------------------------
    def cumulative(self, col, n_rows, op, out=None, out_mask=None, out_device=None):
        """The running fold of one I64 / F64 column on the device (pandrs_hip_cumulative; PandasCompatExt::cumsum / cumprod /
        cummax / cummin / cumcount, src/dataframe/pandas_compat/functions.rs:280-327, :2081-2094): row i covers rows 0 .. i.
        `col` is a (data, mask, dtype) triple on the host or the device, or a ResidentColumn; op is L.CUM_SUM / PROD / MAX /
        MIN / COUNT.  A row under a null bit is skipped: NaN with its bit set (COUNT: the running count, no bit).  `out` /
        `out_mask`: a numpy array or torch CUDA tensor (both in the same space) of at least n_rows float64 (COUNT: int64)
        cells / ceil(n_rows / 8) uint8 to write into.  -> (values, mask, n_null): mask is the uint8 null bitmap of the
        result, None when n_null == 0.  Both are `out` / `out_mask` when given; else torch tensors on this context's device
        for device / resident columns (or out_device=True), else numpy arrays."""
        cc, sp, keep = self._col(col)
        n, op = int(n_rows), int(op)
        out, out_mask, out_device = self._cell_outs(n, sp, op == L.CUM_COUNT, out, out_mask, out_device)
        nulls = C.c_int64(0)
        _check(self.lib.pandrs_hip_cumulative(self.h, sp, cc, n, op, _space(out_device),
                                              _ptr(out) if n else None, _ptr(out_mask) if n else None, C.byref(nulls)))
        return out, (out_mask if nulls.value else None), nulls.value

    def lag(self, col, n_rows, op, periods, out=None, out_mask=None, out_device=None):
        """One I64 / F64 column against itself `periods` rows earlier (pandrs_hip_lag; PandasCompatExt::shift / diff /
        pct_change, functions.rs:328-342, :514-541).  op is L.LAG_SHIFT (any sign of periods; a row without a source, or
        with a null one, is NaN with its bit set), L.LAG_DIFF or L.LAG_PCT_CHANGE (periods >= 0; rows i < periods are NaN
        values with bit 0; a null operand is NaN with its bit set).  Buffers and the result as Context.cumulative; values are
        float64."""
        cc, sp, keep = self._col(col)
        n, op, periods = int(n_rows), int(op), int(periods)
        if not -(1 << 63) <= periods < (1 << 63):
            raise ValueError("periods must fit int64, got %d" % periods)
        out, out_mask, out_device = self._cell_outs(n, sp, False, out, out_mask, out_device)
        nulls = C.c_int64(0)
        _check(self.lib.pandrs_hip_lag(self.h, sp, cc, n, op, C.c_int64(periods), _space(out_device),
                                       _ptr(out) if n else None, _ptr(out_mask) if n else None, C.byref(nulls)))
        return out, (out_mask if nulls.value else None), nulls.value

    def grouped(self, col, n_rows, op, periods=0, out=None, out_mask=None, out_device=None):
        """Context.cumulative / Context.lag within the groups this context retains from its last groupby_indices
        (pandrs_hip_grouped): for every group the ungrouped op over the group's rows in ascending row order, written at those
        rows.  op is L.GROUPED_CUM_SUM / CUM_MAX / CUM_MIN / CUM_COUNT / ROW_NUMBER / SHIFT / DIFF / PCT_CHANGE; `periods` is
        read by the last three.  `col` as Context.cumulative; None for ROW_NUMBER, which reads no column.  n_rows must be the
        grouping's.  Buffers and the result as Context.cumulative; CUM_COUNT and ROW_NUMBER give int64."""
        n, op, periods = int(n_rows), int(op), int(periods)
        if not -(1 << 63) <= periods < (1 << 63):
            raise ValueError("periods must fit int64, got %d" % periods)
        if col is None:
            cc, sp = None, _space(out_device or _is_torch(out))
        else:
            cc, sp, keep = self._col(col)
        out, out_mask, out_device = self._cell_outs(n, sp, op in (L.GROUPED_CUM_COUNT, L.GROUPED_ROW_NUMBER), out, out_mask, out_device)
        nulls = C.c_int64(0)
        _check(self.lib.pandrs_hip_grouped(self.h, sp, cc, n, op, C.c_int64(periods), _space(out_device),
                                           _ptr(out) if n else None, _ptr(out_mask) if n else None, C.byref(nulls)))
        return out, (out_mask if nulls.value else None), nulls.value

    # -- top-k (radix select, compaction, a sort of fewer than k rows) ---------------------------------------------------
    def topk(self, col, n_rows, k, largest=True, out=None, out_device=None):
        """The first min(k, n_rows) rows of one I64 / F64 column in descending (largest) or ascending order on the device
        (pandrs_hip_topk; PandasCompatExt::nlargest / nsmallest, src/dataframe/pandas_compat/functions.rs:159-174): numbers
        by value, ties in row order, then the NaN rows, then the null rows - the first k entries of sort_indices on that
        key.  `col` is a (data, mask, dtype) triple on the host or the device, or a ResidentColumn.  `out`: an int64 numpy
        array or torch CUDA tensor of at least min(k, n_rows) elements to write into.  -> (rows, n_numbers): the int64 row
        indices (`out` when given; else a torch tensor on this context's device for device / resident columns or
        out_device=True, else a numpy array) and how many of them hold a number (they come first)."""
        cc, sp, keep = self._col(col)
        n, k = int(n_rows), int(k)
        kk = max(0, min(k, n))
        out, out_device = self._out_buffer(kk, np.int64, sp, out, out_device, "min(k, n_rows)")
        cnt, num = C.c_int64(0), C.c_int64(0)
        _check(self.lib.pandrs_hip_topk(self.h, sp, cc, n, k, L.TOPK_LARGEST if largest else L.TOPK_SMALLEST,
                                        _space(out_device), _ptr(out) if kk else None, C.byref(cnt), C.byref(num)))
        return out[:cnt.value], num.value

    def arg_extreme(self, col, n_rows):
        """idxmin and idxmax of one I64 / F64 column in one pass on the device (pandrs_hip_arg_extreme; functions.rs:175-192):
        -> (the FIRST row that holds the minimum, the LAST row that holds the maximum), NaN and null cells skipped; None when
        the column holds no number.  `col` as in topk."""
        cc, sp, keep = self._col(col)
        rows = (C.c_int64 * 2)(-1, -1)
        found = C.c_int32(0)
        _check(self.lib.pandrs_hip_arg_extreme(self.h, sp, cc, int(n_rows), rows, C.byref(found)))
        return (int(rows[0]), int(rows[1])) if found.value else None

    # -- row masks (a compare stream, a set probe) ------------------------------------------------------------------------
    def predicate(self, col, n_rows, op, a=0.0, b=0.0, out=None, out_device=None, count_only=False):
        """One row mask of one I64 / F64 column on the device (pandrs_hip_predicate; PandasCompatExt::gt / ge / lt / le /
        eq_value / ne_value / between / is_between / isna / notna / is_finite / is_infinite,
        src/dataframe/pandas_compat/helpers/comparison_ops.rs:7-46, functions.rs:253-257, :4141-4161).  `col` is a (data, mask,
        dtype) triple on the host or the device, or a ResidentColumn; op is L.PRED_*; a and b its f64 arguments (b: the two
        BETWEEN ops).  Every compare happens in f64; a null cell behaves as NaN.  `out`: a uint8 numpy array or torch CUDA
        tensor of at least ceil(n_rows / 8) elements to write into.  -> (bits, count): the LSB-first bitmap, bit = 1 the row
        is selected - the data of a BOOLBITS column, which filter_indices takes as (bits, None, L.BOOLBITS) - and the number
        of set bits.  bits is `out` when given; else a torch tensor on this context's device for device / resident columns
        (or out_device=True), else a numpy array; None with count_only."""
        cc, sp, keep = self._col(col)
        n = int(n_rows)
        out, out_device = self._mask_out(n, sp, out, out_device, count_only)
        cnt = C.c_int64(0)
        _check(self.lib.pandrs_hip_predicate(self.h, sp, cc, n, int(op), float(a), float(b), _space(out_device),
                                             _ptr(out) if n else None, C.byref(cnt)))
        return out, cnt.value

    # -- bins (the edge list from the radix select, one stream for the codes and the counts) ------------------------------
    def bin_edges(self, col, n_rows, kind, k):
        """The reference's edge list of cut (kind L.BIN_CUT, k = bins) or qcut (L.BIN_QCUT, k = q) for one I64 / F64 column
        on the device (pandrs_hip_bin_edges; PandasCompatExt::cut / qcut, src/dataframe/pandas_compat/functions.rs:2349-2351,
        :2392-2397), bit for bit.  `col` is a (data, mask, dtype) triple on the host or the device, or a ResidentColumn.
        -> (k + 1 float64 edges as a numpy array, the number of cells that are neither null nor NaN); no such cell: every
        edge is NaN.  qcut adds 0.001 to the last edge when it looks rows up: that is the caller's step."""
        cc, sp, keep = self._col(col)
        k = int(k)
        out = np.empty(max(k, 0) + 1, np.float64)
        valid = C.c_int64(0)
        _check(self.lib.pandrs_hip_bin_edges(self.h, sp, cc, int(n_rows), int(kind), k, out.ctypes.data_as(C.POINTER(C.c_double)),
                                             C.byref(valid)))
        return out, valid.value

    def bin(self, col, n_rows, edges, out_device=None, want_counts=True, out=None, want_codes=True):
        """The bin of every row of one I64 / F64 column on the device (pandrs_hip_bin): code i where edges[i] <= v <
        edges[i + 1] - the reference's first match, functions.rs:2358-2363 / :2404-2415 - L.BIN_NONE (-1) where no bin
        matches, L.BIN_NAN (-2) for a NaN or null cell.  `edges`: len(edges) - 1 = 1 ... L.BIN_MAX_BINS bins, never
        decreasing, no NaN, +-inf allowed.  `col` as in bin_edges.  `out`: an int32 numpy array or torch CUDA tensor of at
        least n_rows elements to write into.  -> (codes, counts): the int32 codes (`out` when given; else a torch tensor on
        this context's device for device / resident columns or out_device=True, else a numpy array; None with
        want_codes=False) and the int64 rows per code as a numpy array of n_bins + 2, the bins, then NONE, then NAN (None
        with want_counts=False)."""
        cc, sp, keep = self._col(col)
        n = int(n_rows)
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        n_bins = e.shape[0] - 1
        if not want_codes and not want_counts:
            raise ValueError("bin: neither codes nor counts asked for")
        if want_codes:
            out, out_device = self._out_buffer(n, np.int32, sp, out, out_device, "n_rows")
        elif out is not None:
            raise ValueError("want_codes=False takes no out")
        else:
            out_device = False
        # (no rows: no codes pointer is passed, so the counts stand for "something asked for")
        counts = np.zeros(max(n_bins, 0) + 2, np.int64) if want_counts or n == 0 else None
        _check(self.lib.pandrs_hip_bin(self.h, sp, cc, n, e.ctypes.data_as(C.POINTER(C.c_double)), n_bins, _space(out_device),
                                       _ptr(out) if n and out is not None else None,
                                       None if counts is None else counts.ctypes.data_as(C.POINTER(C.c_int64))))
        return out, (counts if want_counts else None)

    # -- distinct values and their counts (an LDS table for few distinct integers, else the groupby engine) ----------------
    def distinct(self, col, n_rows, order, code_rank=None, out_device=False):
        """The distinct values of one I64 / F64 / U32CODE / BOOLBITS column and how often each occurs, on the device
        (pandrs_hip_distinct + pandrs_hip_distinct_fetch; PandasCompatExt::value_counts / unique / nunique / mode,
        src/dataframe/pandas_compat/functions.rs:343-384, :1709-1753, :4120-4139).  `col` is a (data, mask, dtype) triple on the
        host or the device, or a ResidentColumn; `order` L.DISTINCT_BY_VALUE (numbers ascending, -0.0 before 0.0, then the NaN
        entry, then the NULL entry) or L.DISTINCT_BY_COUNT (count descending, ties in that order); `code_rank` the string
        pool's rank table, which makes a U32CODE column order by its strings instead of its codes.
        -> (values, flags, counts, info): uint64 cells (the i64, the f64 bits, the code, 0 / 1), uint8 flags (L.DISTINCT_NUMBER,
        L.DISTINCT_NAN, L.DISTINCT_NULL), exact int64 counts - numpy arrays, or with out_device torch tensors on this context's
        device (values as int64 bit patterns) - and the L.DistinctInfo of the call as a dict."""
        cc, sp, keep = self._col(col)
        rank, n_codes = self._code_rank(code_rank, sp, keep)
        info = L.DistinctInfo()
        _check(self.lib.pandrs_hip_distinct(self.h, sp, cc, int(n_rows), int(order), _ptr(rank), n_codes, C.byref(info)))
        values, flags, counts = self.distinct_fetch(info.n_entries, out_device)
        return values, flags, counts, {name: getattr(info, name) for name, _ in L.DistinctInfo._fields_ if name != "reserved"}

    def distinct_fetch(self, n_entries, out_device=False, values=True, flags=True, counts=True):
        """The list the last distinct call left in the context (until the next compute call on it), or the parts asked for."""
        n = int(n_entries)
        v = self._empty(n, np.uint64, out_device) if values else None
        f = self._empty(n, np.uint8, out_device) if flags else None
        k = self._empty(n, np.int64, out_device) if counts else None
        _check(self.lib.pandrs_hip_distinct_fetch(self.h, _space(out_device), _ptr(v) if n else None,
                                                  _ptr(f) if n else None, _ptr(k) if n else None))
        return v, f, k

    # -- a group-by over two key columns as a dense matrix (one fused stream into an LDS table, else the groupby engine) -----
    def pivot(self, index_col, columns_col, n_rows, op, values_col=None, index_rank=None, columns_rank=None, out_device=False):
        """The two-key group-by of (index_col, columns_col) laid out as an R x C matrix, on the device (pandrs_hip_pivot +
        pandrs_hip_pivot_fetch; crosstab, src/dataframe/pandas_compat/functions.rs:2138-2183; pivot_table, src/pivot/mod.rs:12-250;
        pivot / unstack, functions.rs:2471-2527).  The key columns are (data, mask, dtype) triples of I64 / F64 / U32CODE /
        BOOLBITS, all on the host or all on the device, or ResidentColumns; `op` an L.PIVOT_* number; `values_col` an I64 / F64
        column, None for L.PIVOT_ROWS; `index_rank` / `columns_rank` the string pool's rank table, which makes a U32CODE key
        order its labels by their strings instead of their codes.
        -> (index_labels, index_flags, column_labels, column_flags, cells, rows, info): uint64 label cells (the i64, the f64
        bits, the code, 0 / 1) ascending, uint8 flags (1 = the one missing label, last), the cells as a float64 (C, R) array
        - cells[j, i] belongs to index label i and columns label j, NaN where no row holds the pair - the exact int64 rows per
        cell in the same shape, numpy arrays or with out_device torch tensors on this context's device (labels as int64 bit
        patterns), and the L.PivotInfo of the call as a dict."""
        cols = [tuple(index_col), tuple(columns_col)] + ([tuple(values_col)] if values_col is not None else [])
        keep = []
        cc, sp = self._cols(cols, keep)
        rank1, n_codes1 = self._code_rank(index_rank, sp, keep)
        rank2, n_codes2 = self._code_rank(columns_rank, sp, keep)
        info = L.PivotInfo()
        at = lambda i: C.cast(C.byref(cc, i * C.sizeof(L.Column)), C.POINTER(L.Column))        # noqa: E731
        _check(self.lib.pandrs_hip_pivot(self.h, sp, at(0), _ptr(rank1), n_codes1, at(1), _ptr(rank2), n_codes2,
                                         at(2) if values_col is not None else None, int(n_rows), int(op), C.byref(info)))
        out = self.pivot_fetch(info.n_index_labels, info.n_column_labels, out_device)
        return out + ({name: getattr(info, name) for name, _ in L.PivotInfo._fields_ if name != "reserved"},)

    def pivot_fetch(self, n_index_labels, n_column_labels, out_device=False, labels=True, cells=True, rows=True):
        """The result the last pivot call left in the context (until the next compute call on it), or the parts asked for."""
        r, c = int(n_index_labels), int(n_column_labels)
        il = self._empty(r, np.uint64, out_device) if labels else None
        fi = self._empty(r, np.uint8, out_device) if labels else None
        cl = self._empty(c, np.uint64, out_device) if labels else None
        fc = self._empty(c, np.uint8, out_device) if labels else None
        ce = self._empty((c, r), np.float64, out_device) if cells else None
        ro = self._empty((c, r), np.int64, out_device) if rows else None
        some = r > 0 and c > 0
        _check(self.lib.pandrs_hip_pivot_fetch(self.h, _space(out_device), *[_ptr(x) if some else None for x in (il, fi, cl, fc, ce, ro)]))
        return il, fi, cl, fc, ce, ro

    # -- derived columns (one postfix program over up to eight columns, one stream) ---------------------------------------
    @staticmethod
    def eval_check(dtypes, program):
        """The validator of pandrs_hip_eval without a context or a device (pandrs_hip_eval_check).  `dtypes`: the dtype of
        every column; `program`: (op, arg) pairs in postfix order, op an L.EVAL_* number, arg the column index of COL and the
        constant of CONST.  -> (is_mask, depth); raises what the call itself would."""
        program = list(program)
        ops, args = Context._program(program)
        return Context._eval_check(dtypes, ops, args, len(program))

    @staticmethod
    def _eval_check(dtypes, ops, args, n_ops):
        dts = (C.c_int32 * max(len(dtypes), 1))(*[int(d) for d in dtypes])
        is_mask, depth = C.c_int32(0), C.c_int32(0)
        _check(L.load().pandrs_hip_eval_check(dts, len(dtypes), ops, args, n_ops, C.byref(is_mask), C.byref(depth)))
        return bool(is_mask.value), depth.value

    @staticmethod
    def _program(program):
        ops = (C.c_int32 * max(len(program), 1))(*[int(op) for op, _ in program])
        args = (C.c_double * max(len(program), 1))(*[float(arg) for _, arg in program])
        return ops, args

    def eval(self, cols, n_rows, program, out=None, out_mask=None, out_device=None):
        """One postfix program over up to eight columns, evaluated per row in one stream (pandrs_hip_eval): what
        PandasCompatExt::add_scalar .. div_scalar / col_add .. col_div / clip / where_cond / round / coalesce and the like
        (functions.rs:2819-2960, :237, :1079-1139, helpers/math_ops.rs) compute, and any expression over them, at the cost of
        its algorithmic bytes.  `cols`: (data, mask, dtype) triples, all on the host or all on the device, or ResidentColumns
        (I64, F64 or BOOLBITS); `program`: (op, arg) pairs as in eval_check.  Every operation is rounded on its own; a numeric
        cell under a null bit loads as NaN, a boolean one as false.
        A value program -> (values, mask, n_null) as Context.lag: float64 cells, every NaN canonical; a null bit where the
        result is NaN and a named cell of the row was null.  A boolean program -> (bits, count) as Context.predicate: the
        LSB-first bitmap filter_indices takes as (bits, None, L.BOOLBITS); `out` is then the uint8 bitmap and out_mask must be
        None.  Results are `out` / `out_mask` when given; else torch tensors on this context's device for device / resident
        columns (or out_device=True), else numpy arrays."""
        cols, program = [tuple(c) for c in cols], list(program)
        ops, args = self._program(program)
        is_mask, _ = self._eval_check([c[2] for c in cols], ops, args, len(program))
        keep = []
        cc, sp = self._cols(cols, keep)
        n = int(n_rows)
        cnt = C.c_int64(0)
        if is_mask:
            if out_mask is not None:
                raise ValueError("a boolean program takes no out_mask")
            out, out_device = self._out_buffer((n + 7) // 8, np.uint8, sp, out, out_device, "ceil(n_rows / 8)")
        else:
            out, out_mask, out_device = self._cell_outs(n, sp, False, out, out_mask, out_device)
        _check(self.lib.pandrs_hip_eval(self.h, sp, cc, len(cols), n, ops, args, len(program), _space(out_device),
                                        _ptr(out) if n else None, _ptr(out_mask) if n else None, C.byref(cnt)))
        if is_mask:
            return out, cnt.value
        return out, (out_mask if cnt.value else None), cnt.value

    def isin(self, col, n_rows, values, negate=False, out=None, out_device=None, count_only=False):
        """Membership of every cell of one column in a value list on the device (pandrs_hip_isin; PandasCompatExt::isin /
        isin_numeric, functions.rs:141-158): cells are compared by their bits (-0.0 is not 0.0, a NaN matches the same payload
        only).  `col` as in predicate, also U32CODE; `values` is a (data, None, dtype) triple on the host or the device (its
        space is independent of the column's): F64 / F64, I64 / F64 (the cell as f64), I64 / I64 (as integers) or U32CODE /
        U32CODE.  A null cell never matches; `negate` inverts every bit.  -> (bits, count) as predicate."""
        cc, sp, keep = self._col(col)
        vdata, vmask, vdt = tuple(values)
        if vmask is not None:
            raise ValueError("the value list takes no null mask")
        n_values = int(vdata.numel() if _is_torch(vdata) else np.asarray(vdata).shape[0])
        vc, vsp = self._cols([(vdata, None, vdt)], keep)
        n = int(n_rows)
        out, out_device = self._mask_out(n, sp, out, out_device, count_only)
        cnt = C.c_int64(0)
        _check(self.lib.pandrs_hip_isin(self.h, sp, cc, n, vsp, vc, n_values, 1 if negate else 0, _space(out_device),
                                        _ptr(out) if n else None, C.byref(cnt)))
        return out, cnt.value
