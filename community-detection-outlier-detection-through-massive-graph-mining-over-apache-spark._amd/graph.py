"""Low-level handle over liblpa_hip.so: one built graph on one GPU (or one rank's slice).

Inputs are dense int32 edge arrays: host numpy arrays, or device tensors (any
object with ``data_ptr()`` and ``is_cuda``, e.g. torch-ROCm tensors), which are
handed to the C ABI as plain device pointers (torch is only the allocator).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

OUTLIER_MODES = {"L1": 1, "L2": 2, 1: 1, 2: 2}


def _is_device_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _edge_ptrs(src, dst):
    """Returns (src_ptr, dst_ptr, m, flags, keepalive)."""
    if _is_device_tensor(src) != _is_device_tensor(dst):
        raise ValueError("src and dst must both be host arrays or both device tensors")
    if _is_device_tensor(src):
        import torch

        if src.dtype != torch.int32 or dst.dtype != torch.int32:
            raise ValueError("device edge tensors must be int32")
        if src.numel() != dst.numel():
            raise ValueError("src/dst length mismatch")
        src = src.contiguous()
        dst = dst.contiguous()
        torch.cuda.current_stream(src.device).synchronize()
        return src.data_ptr(), dst.data_ptr(), int(src.numel()), _lib.LPA_INPUT_DEVICE, (src, dst)
    s = np.ascontiguousarray(src, dtype=np.int32)
    d = np.ascontiguousarray(dst, dtype=np.int32)
    if s.shape != d.shape or s.ndim != 1:
        raise ValueError("src/dst must be 1-D arrays of equal length")
    return s.ctypes.data, d.ctypes.data, int(s.size), 0, (s, d)


# role codes of Graph.scan / lpa_scan, by value
SCAN_ROLES = ("outlier", "hub", "border", "core")


def _check_scan(eps, mu, eps_name="eps"):
    """The argument checks of Graph.scan and GraphFrame.scan, before any device work; returns
    (float eps, int mu)."""
    if isinstance(eps, (bool, np.bool_)) or not isinstance(eps, (int, float, np.integer, np.floating)):
        raise TypeError(f"{eps_name} must be a real number, got {type(eps).__name__}")
    if not isinstance(mu, (int, np.integer)) or isinstance(mu, (bool, np.bool_)):
        raise TypeError(f"mu must be an int, got {type(mu).__name__}")
    if not 0 < eps <= 1:   # NaN fails both
        raise ValueError(f"{eps_name} must belong to (0, 1], but got {eps}")
    if mu < 1:
        raise ValueError(f"mu must be at least 1, but got {mu}")
    return float(eps), min(int(mu), 2 ** 31 - 1)


class PregelNullError(ValueError):
    """An initial (``iteration`` 0) or updated value of Pregel column ``column`` was null at the
    dense vertex ``vertex``: a column holds no null."""

    def __init__(self, msg, iteration, column, vertex):
        super().__init__(msg)
        self.iteration, self.column, self.vertex = iteration, column, vertex


class Graph:
    """A symmetrised, degree-sorted CSR resident in HBM plus its label vectors.

    ``Graph(src, dst, V)`` builds on ``device``; ``Graph(..., rank=r, nranks=P,
    comm_id=id)`` builds rank r's slice for a P-GPU run (one process per GPU,
    RCCL allgather per superstep); ``Graph(..., rank=r, loopback=group)`` builds
    rank r of an in-process ``Loopback`` group (P handles on one device, one host
    thread each, the same exchange code with D2D copies for the allgather);
    ``comm_id=None`` with ``nranks > 1`` selects the caller-driven exchange
    (``exchange_get`` / ``exchange_put``); ``allgather=fn`` the host-staged collective
    (``lpa_graph_create_hostcoll``): the library's own exchange schedule with every
    allgather done by ``fn(send: np.ndarray[uint8]) -> bytes-like of nranks * send.size``
    (e.g. torch.distributed gloo between processes).
    """

    def __init__(self, src, dst, num_vertices: int, device: int = 0, rank: int = 0,
                 nranks: int = 1, comm_id: bytes | None = None, loopback: "Loopback | None" = None,
                 allgather=None):
        lib = _lib.load()
        self._lib = lib
        self._h = ctypes.c_void_p()
        self._allgather_cb = None
        self._allgather_err = None
        sp, dp, m, flags, keep = _edge_ptrs(src, dst)
        V = int(num_vertices)
        if V < 0 or V > np.iinfo(np.int32).max:
            raise ValueError(f"num_vertices out of range: {V}")
        if allgather is not None:
            P = int(nranks)

            def _cb(send, recv, nbytes, _ctx):
                try:
                    n = int(nbytes)
                    src_b = np.ctypeslib.as_array((ctypes.c_uint8 * max(n, 1)).from_address(send))[:n]
                    out = np.frombuffer(memoryview(allgather(src_b.copy())), dtype=np.uint8)
                    if out.size != P * n:
                        raise ValueError(f"allgather returned {out.size} bytes, expected {P * n}")
                    if n > 0:
                        ctypes.memmove(recv, out.ctypes.data, P * n)
                    return 0
                except BaseException as e:  # noqa: BLE001 -- reported after the failed call
                    self._allgather_err = e
                    return -1

            self._allgather_cb = _lib.ALLGATHER_FN(_cb)   # kept alive with the handle
            rc = lib.lpa_graph_create_hostcoll(sp, dp, m, V, device, flags, rank, P, self._allgather_cb, None,
                                               ctypes.byref(self._h))
        elif loopback is not None:
            nranks = loopback.nranks
            rc = lib.lpa_graph_create_loopback(sp, dp, m, V, device, flags, rank, loopback._handle(),
                                               ctypes.byref(self._h))
        elif nranks == 1 and comm_id is None:
            rc = lib.lpa_graph_create(sp, dp, m, V, device, flags, ctypes.byref(self._h))
        else:
            cid = None if comm_id is None else bytes(comm_id)
            if cid is not None and len(cid) != 128:
                raise ValueError("comm_id must be 128 bytes")
            rc = lib.lpa_graph_create_dist(sp, dp, m, V, device, flags, rank, nranks, cid,
                                           ctypes.byref(self._h))
        del keep
        _lib.check(rc)
        self.num_vertices = V
        self.num_edges = m
        self.device = device
        self.rank = rank
        self.nranks = nranks
        self._loopback = loopback   # the group must outlive the handle

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if self._h:
            self._lib.lpa_graph_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._h:
            raise ValueError("graph handle is closed")
        return self._h

    def _check(self, rc: int):
        """check() that re-raises a host allgather function's own exception as the cause."""
        err, self._allgather_err = self._allgather_err, None
        if rc != _lib.LPA_OK and err is not None:
            raise _lib.LpaError(rc, _lib.last_error()) from err
        _lib.check(rc)

    # -- LPA ----------------------------------------------------------------
    def info(self) -> dict:
        info = _lib.LpaGraphInfo()
        _lib.check(self._lib.lpa_graph_get_info_sized(self._handle(), ctypes.byref(info), ctypes.sizeof(info)))
        return info.to_dict()

    def reset(self):
        _lib.check(self._lib.lpa_reset(self._handle()))

    def step(self, n: int = 1, stats: bool = False):
        st = _lib.LpaStats() if stats else None
        self._check(self._lib.lpa_step(self._handle(), int(n), ctypes.byref(st) if stats else None))
        return st.to_dict() if stats else None

    def labels(self, out=None) -> np.ndarray:
        """Current labels by dense vertex id (host int32), or into a device tensor `out`."""
        if out is not None and _is_device_tensor(out):
            _lib.check(self._lib.lpa_get_labels(self._handle(), out.data_ptr(), 1))
            return out
        lab = np.empty(self.num_vertices, dtype=np.int32)
        _lib.check(self._lib.lpa_get_labels(self._handle(), lab.ctypes.data, 0))
        return lab

    def run(self, max_iter: int, stats: bool = False, out=None):
        """labelPropagation(maxIter): reset, exactly max_iter supersteps, labels
        (host int32 array, or written into the device tensor ``out``)."""
        st = _lib.LpaStats() if stats else None
        if out is not None and _is_device_tensor(out):
            if out.numel() != self.num_vertices:
                raise ValueError(f"out must hold {self.num_vertices} labels")
            lab, ptr, on_dev = out, out.data_ptr(), 1
        else:
            lab = np.empty(self.num_vertices, dtype=np.int32)
            ptr, on_dev = lab.ctypes.data, 0
        self._check(self._lib.lpa_run(self._handle(), int(max_iter), ptr, on_dev,
                                      ctypes.byref(st) if stats else None))
        return (lab, st.to_dict()) if stats else lab

    def degrees(self) -> np.ndarray:
        deg = np.empty(self.num_vertices, dtype=np.int32)
        _lib.check(self._lib.lpa_degrees(self._handle(), deg.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return deg

    def set_frontier(self, on: bool = True):
        """Re-tally only rows with a changed neighbour (exact; default on) or every row."""
        _lib.check(self._lib.lpa_set_frontier(self._handle(), int(bool(on))))

    def set_posted(self, cap: int = -1):
        """P > 1: posted delta exchange capacity (-1 adaptive, 0 off, > 0 fixed; labels identical)."""
        _lib.check(self._lib.lpa_set_posted(self._handle(), int(cap)))

    def set_serial(self, serial: bool = True):
        """Profiling: queue every tally kernel on one stream (standalone kernel times)."""
        _lib.check(self._lib.lpa_set_serial(self._handle(), int(bool(serial))))

    # -- caller-driven exchange (virtual ranks) -------------------------------
    def exchange_get(self) -> np.ndarray:
        sl = np.empty(self.info()["slice"], dtype=np.int32)
        _lib.check(self._lib.lpa_exchange_get(self._handle(), sl.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return sl

    def exchange_put(self, full: np.ndarray):
        full = np.ascontiguousarray(full, dtype=np.int32)
        _lib.check(self._lib.lpa_exchange_put(self._handle(), full.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))

    def exchange_get_delta(self) -> np.ndarray:
        """This rank's changed owned labels as (local slot << 32 | label) entries."""
        buf = np.empty(max(self.info()["slice"], 1), dtype=np.uint64)
        n = ctypes.c_int64(0)
        _lib.check(self._lib.lpa_exchange_get_delta(self._handle(), buf.ctypes.data_as(ctypes.c_void_p),
                                                    ctypes.byref(n)))
        return buf[: n.value].copy()

    def exchange_put_delta(self, per_rank):
        """Apply every rank's delta entries (list in rank order)."""
        cap = max((e.size for e in per_rank), default=0)
        P = len(per_rank)
        table = np.zeros((P, max(cap, 1)), dtype=np.uint64)
        for r, e in enumerate(per_rank):
            table[r, : e.size] = e
        counts = np.array([e.size for e in per_rank], dtype=np.int64)
        _lib.check(self._lib.lpa_exchange_put_delta(self._handle(), table.ctypes.data_as(ctypes.c_void_p),
                                                    counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                    cap))

    # -- outlier stage --------------------------------------------------------
    def outlier(self, labels, mode="L1", sub_iter: int = 5):
        """Appendix B outlier stage.  Returns dict(size, incident, sub_labels, flags, summary):
        host numpy arrays for host labels; for a device label tensor (int32, this
        handle's device) every output is a device tensor of this device and nothing is
        staged through the host (lpa_outlier_device)."""
        if mode not in OUTLIER_MODES:
            raise ValueError(f"mode must be 'L1' or 'L2', got {mode!r}")
        md = OUTLIER_MODES[mode]
        V = self.num_vertices
        if _is_device_tensor(labels):
            return self._outlier_device(labels, md, sub_iter)
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.shape != (V,):
            raise ValueError(f"labels must have shape ({V},)")
        size = np.empty(V, dtype=np.int64)
        inc = np.empty(V, dtype=np.int64)
        sub = np.empty(V, dtype=np.int32) if md == 2 else None
        flags = np.empty(V, dtype=np.uint8)
        summ = _lib.LpaOutlierSummary()
        i64p = ctypes.POINTER(ctypes.c_int64)
        _lib.check(self._lib.lpa_outlier(
            self._handle(), lab.ctypes.data, 0, md, int(sub_iter),
            size.ctypes.data_as(i64p), inc.ctypes.data_as(i64p),
            sub.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if sub is not None else None,
            flags.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(summ)))
        return dict(size=size, incident=inc, sub_labels=sub, flags=flags.astype(bool),
                    summary=summ.to_dict())


    def _outlier_device(self, labels, md: int, sub_iter: int):
        import torch

        V = self.num_vertices
        if labels.dtype != torch.int32:
            raise ValueError(f"device labels must be int32, got {labels.dtype}")
        if labels.device.index != self.device:
            raise ValueError(f"device labels must be on cuda:{self.device}, got {labels.device}")
        if labels.numel() != V:
            raise ValueError(f"labels must hold {V} entries")
        lab = labels.contiguous()
        dev = lab.device
        size = torch.empty(V, dtype=torch.int64, device=dev)
        inc = torch.empty(V, dtype=torch.int64, device=dev)
        sub = torch.empty(V, dtype=torch.int32, device=dev) if md == 2 else None
        flags = torch.empty(V, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()   # the library works on its own stream
        summ = _lib.LpaOutlierSummary()
        _lib.check(self._lib.lpa_outlier_device(
            self._handle(), lab.data_ptr(), md, int(sub_iter), size.data_ptr(), inc.data_ptr(),
            sub.data_ptr() if sub is not None else None, flags.data_ptr(), ctypes.byref(summ)))
        return dict(size=size, incident=inc, sub_labels=sub, flags=flags.bool(), summary=summ.to_dict())

    def quality(self, labels) -> dict:
        """Community count and modularity of a labelling (host array or device tensor of
        dense-id labels) on this graph's symmetrised multigraph (lpa_quality)."""
        q = _lib.LpaQualitySummary()
        if _is_device_tensor(labels):
            import torch

            # the library reads V int32 values on its own stream (as _edge_ptrs guards the
            # edge tensors): wrong dtype / device would be read silently, an unfinished
            # producer on torch's stream too early
            if labels.dtype != torch.int32:
                raise ValueError(f"device labels must be int32, got {labels.dtype}")
            if labels.device.index != self.device:
                raise ValueError(f"device labels must be on cuda:{self.device}, got {labels.device}")
            if labels.numel() != self.num_vertices:
                raise ValueError(f"labels must hold {self.num_vertices} entries")
            lab, on_dev = labels.contiguous(), 1
            torch.cuda.current_stream(lab.device).synchronize()
            ptr = lab.data_ptr()
        else:
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            if lab.shape != (self.num_vertices,):
                raise ValueError(f"labels must have shape ({self.num_vertices},)")
            ptr, on_dev = lab.ctypes.data, 0
        _lib.check(self._lib.lpa_quality(self._handle(), ptr, on_dev, ctypes.byref(q)))
        return q.to_dict()

    # -- connected components ---------------------------------------------------
    def components(self, out=None, sizes: bool = False):
        """Connected components of the undirected view of the input multigraph
        (lpa_components): ``comp[v]`` is the smallest dense id of v's component.  Host int32
        array by default, or written into the int32 device tensor ``out`` (this handle's
        device, ``num_vertices`` entries).  ``sizes=True`` returns ``(comp, sizes, summary)``:
        ``sizes[c]`` (int64, in the memory ``comp`` is in) holds the member count at every
        component id c and 0 elsewhere; ``summary`` is a dict of n_components, n_singletons,
        largest_size, largest_id.  The labels and the LPA state are not touched."""
        V = self.num_vertices
        size = None
        if out is not None and _is_device_tensor(out):
            import torch

            if out.dtype != torch.int32:
                raise ValueError(f"out must be int32, got {out.dtype}")
            if out.device.index != self.device:
                raise ValueError(f"out must be on cuda:{self.device}, got {out.device}")
            if out.numel() != V or not out.is_contiguous():
                raise ValueError(f"out must hold {V} contiguous entries")
            comp, ptr, on_dev = out, out.data_ptr(), 1
            if sizes:
                size = torch.empty(V, dtype=torch.int64, device=out.device)
            torch.cuda.current_stream(out.device).synchronize()   # the library works on its own stream
            size_ptr = size.data_ptr() if sizes else None
        elif out is not None:
            raise ValueError("out must be an int32 device tensor")
        else:
            comp = np.empty(V, dtype=np.int32)
            ptr, on_dev = comp.ctypes.data, 0
            if sizes:
                size = np.empty(V, dtype=np.int64)
            size_ptr = size.ctypes.data if sizes else None
        summ = _lib.LpaComponentsSummary()
        _lib.check(self._lib.lpa_components(self._handle(), ptr, on_dev, size_ptr,
                                            ctypes.byref(summ) if sizes else None))
        return (comp, size, summ.to_dict()) if sizes else comp

    # -- triangles ----------------------------------------------------------------
    def triangle_count(self, out=None, stats: bool = False):
        """Triangles per vertex of the canonical simple undirected graph of the input
        multigraph (lpa_triangle_count: self-loops dropped, direction ignored, duplicates
        collapsed): ``count[v]`` is the number of triangles that contain v.  Host int64
        array by default, or written into the int64 device tensor ``out`` (this handle's
        device, ``num_vertices`` entries).  ``stats=True`` returns ``(count, simple_degree,
        summary)``: ``simple_degree[v]`` (int64, in the memory ``count`` is in) is the number
        of distinct neighbours of v; ``summary`` is a dict of n_triangles, simple_edges,
        wedges, n_in_triangle, max_count, max_count_id.  The labels and the LPA state are
        not touched."""
        V = self.num_vertices
        deg = None
        if out is not None and _is_device_tensor(out):
            import torch

            if out.dtype != torch.int64:
                raise ValueError(f"out must be int64, got {out.dtype}")
            if out.device.index != self.device:
                raise ValueError(f"out must be on cuda:{self.device}, got {out.device}")
            if out.numel() != V or not out.is_contiguous():
                raise ValueError(f"out must hold {V} contiguous entries")
            count, ptr, on_dev = out, out.data_ptr(), 1
            if stats:
                deg = torch.empty(V, dtype=torch.int64, device=out.device)
            torch.cuda.current_stream(out.device).synchronize()   # the library works on its own stream
            deg_ptr = deg.data_ptr() if stats else None
        elif out is not None:
            raise ValueError("out must be an int64 device tensor")
        else:
            count = np.empty(V, dtype=np.int64)
            ptr, on_dev = count.ctypes.data, 0
            if stats:
                deg = np.empty(V, dtype=np.int64)
            deg_ptr = deg.ctypes.data if stats else None
        summ = _lib.LpaTriangleSummary()
        _lib.check(self._lib.lpa_triangle_count(self._handle(), ptr, deg_ptr, on_dev,
                                                ctypes.byref(summ) if stats else None))
        return (count, deg, summ.to_dict()) if stats else count

    # -- PageRank -----------------------------------------------------------------
    def pagerank(self, max_iter: int, reset_prob: float = 0.15, source=None, out=None, stats: bool = False):
        """Static PageRank of the directed input multigraph (lpa_pagerank; GraphX
        ``PageRank.runWithOptions``): exactly ``max_iter`` supersteps from rank 1.0, every
        kept edge u -> v weighted 1 / outdeg[u] (duplicates are edges), then normalised to
        sum to ``num_vertices``.  ``source`` (a dense id): the personalised form, which
        starts and resets at that vertex only and sums to 1.  Host float64 array by default,
        or written into the float64 device tensor ``out`` (this handle's device,
        ``num_vertices`` entries).  ``stats=True`` returns ``(rank, out_degree, in_degree,
        summary)``: the degrees (int64, in the memory ``rank`` is in) count duplicates;
        ``summary`` is a dict of rank_sum (before normalisation), max_rank, max_rank_id,
        edges, sinks, max_in_degree.  The ranks are bit-identical across runs, handles and
        input edge orders.  The labels and the LPA state are not touched."""
        if not isinstance(max_iter, (int, np.integer)) or isinstance(max_iter, bool):
            raise TypeError(f"max_iter must be an int, got {type(max_iter).__name__}")
        if source is not None and (not isinstance(source, (int, np.integer)) or isinstance(source, bool)):
            raise TypeError(f"source must be a dense vertex id or None, got {type(source).__name__}")
        V = self.num_vertices
        src = -1 if source is None else int(source)
        if source is not None and not 0 <= src < V:
            raise ValueError(f"source {src} is not a vertex of [0, {V})")
        odeg = ideg = None
        if out is not None and _is_device_tensor(out):
            import torch

            if out.dtype != torch.float64:
                raise ValueError(f"out must be float64, got {out.dtype}")
            if out.device.index != self.device:
                raise ValueError(f"out must be on cuda:{self.device}, got {out.device}")
            if out.numel() != V or not out.is_contiguous():
                raise ValueError(f"out must hold {V} contiguous entries")
            rank, ptr, on_dev = out, out.data_ptr(), 1
            if stats:
                odeg = torch.empty(V, dtype=torch.int64, device=out.device)
                ideg = torch.empty(V, dtype=torch.int64, device=out.device)
            torch.cuda.current_stream(out.device).synchronize()   # the library works on its own stream
            odeg_ptr, ideg_ptr = (odeg.data_ptr(), ideg.data_ptr()) if stats else (None, None)
        elif out is not None:
            raise ValueError("out must be a float64 device tensor")
        else:
            rank = np.empty(V, dtype=np.float64)
            ptr, on_dev = rank.ctypes.data, 0
            if stats:
                odeg = np.empty(V, dtype=np.int64)
                ideg = np.empty(V, dtype=np.int64)
            odeg_ptr, ideg_ptr = (odeg.ctypes.data, ideg.ctypes.data) if stats else (None, None)
        summ = _lib.LpaPagerankSummary()
        _lib.check(self._lib.lpa_pagerank(self._handle(), int(max_iter), float(reset_prob), src, ptr, odeg_ptr,
                                          ideg_ptr, on_dev, ctypes.byref(summ) if stats else None))
        return (rank, odeg, ideg, summ.to_dict()) if stats else rank

    # -- parallel personalized PageRank -------------------------------------------------
    def parallel_pagerank(self, sources, max_iter: int, reset_prob: float = 0.15, out=None, stats: bool = False):
        """Personalised PageRank from every one of ``sources`` (dense ids) in one call
        (lpa_parallel_pagerank; GraphX ``PageRank.runParallelPersonalizedPageRank``): row l of
        the result is what ``pagerank(max_iter, reset_prob, source=sources[l])`` specifies, each
        row summing to 1.  The in-list CSR is built once and the sources run ``batch_width`` to a
        pass (``LPA_PPR_BATCH`` = 4, 8 or 16 when the handle is created), one gathered in-edge
        serving the whole pass.  A source may repeat: its rows are then equal (GraphX keeps
        only the last of a repeat and returns 0 / 0 for the earlier ones; that accident is not
        reproduced).  Host float64 array of shape ``(len(sources), num_vertices)`` by default,
        or written into the contiguous float64 device tensor ``out`` of that shape (this
        handle's device).  ``stats=True`` returns ``(ranks, rank_sums, summary)``:
        ``rank_sums[l]`` (host float64) is row l's sum before normalisation, ``summary`` a dict
        of edges, sinks, max_in_degree, batches, batch_width, nonzero, rank_sum_min,
        rank_sum_max.  A row is bit-identical across runs, handles, input edge orders, the
        position of its source in ``sources`` and whatever other sources share the call; it
        agrees with ``pagerank``'s personalised ranks within that call's bound, not bit for
        bit.  The labels and the LPA state are not touched."""
        if not isinstance(max_iter, (int, np.integer)) or isinstance(max_iter, (bool, np.bool_)):
            raise TypeError(f"max_iter must be an int, got {type(max_iter).__name__}")
        srcs = list(sources) if not isinstance(sources, (str, bytes)) else [sources]
        for x in srcs:
            if not isinstance(x, (int, np.integer)) or isinstance(x, (bool, np.bool_)):
                raise TypeError(f"a source must be a dense vertex id (int), got {type(x).__name__}")
        V = self.num_vertices
        for x in srcs:
            if not 0 <= int(x) < V:
                raise ValueError(f"source {int(x)} is not a vertex of [0, {V})")
        n = len(srcs)
        sv = np.asarray(srcs, dtype=np.int32).reshape(n)
        if out is not None and _is_device_tensor(out):
            import torch

            if out.dtype != torch.float64:
                raise ValueError(f"out must be float64, got {out.dtype}")
            if out.device.index != self.device:
                raise ValueError(f"out must be on cuda:{self.device}, got {out.device}")
            if tuple(out.shape) != (n, V) or not out.is_contiguous():
                raise ValueError(f"out must hold ({n}, {V}) contiguous entries")
            ranks, ptr, on_dev = out, out.data_ptr(), 1
            torch.cuda.current_stream(out.device).synchronize()   # the library works on its own stream
        elif out is not None:
            raise ValueError("out must be a float64 device tensor")
        else:
            ranks = np.empty((n, V), dtype=np.float64)
            ptr, on_dev = ranks.ctypes.data, 0
        sums = np.empty(n, dtype=np.float64)
        summ = _lib.LpaPprSummary()
        _lib.check(self._lib.lpa_parallel_pagerank(self._handle(), int(max_iter), float(reset_prob),
                                                   sv.ctypes.data_as(_lib._i32p), n, ptr, on_dev,
                                                   sums.ctypes.data if stats else None,
                                                   ctypes.byref(summ) if stats else None))
        return (ranks, sums, summ.to_dict()) if stats else ranks

    # -- shortest paths -------------------------------------------------------------
    def shortest_paths(self, landmarks, out=None, stats: bool = False):
        """Landmark shortest paths of the directed input graph (lpa_shortest_paths; GraphX
        ``lib.ShortestPaths``): ``dist[l, v]`` is the number of edges on a shortest directed
        path from v to ``landmarks[l]`` along src -> dst, 0 at the landmark, -1 where there is
        none.  Duplicate edges and self-loops change nothing.  ``landmarks``: dense ids, a
        landmark may repeat (equal rows).  Host int32 array of shape ``(len(landmarks),
        num_vertices)`` by default, or written into the contiguous int32 device tensor ``out``
        of that shape (this handle's device).  ``stats=True`` returns ``(dist, summary)``:
        ``summary`` is a dict of arcs, reached, max_distance, batches, push_levels,
        pull_levels.  The distances are identical across runs, handles, input edge orders
        and push / pull schedules.  The labels and the LPA state are not touched."""
        lms = list(landmarks) if not isinstance(landmarks, (str, bytes)) else [landmarks]
        for x in lms:
            if not isinstance(x, (int, np.integer)) or isinstance(x, (bool, np.bool_)):
                raise TypeError(f"a landmark must be a dense vertex id (int), got {type(x).__name__}")
        V = self.num_vertices
        for x in lms:
            if not 0 <= int(x) < V:
                raise ValueError(f"landmark {int(x)} is not a vertex of [0, {V})")
        n = len(lms)
        lm = np.asarray(lms, dtype=np.int32).reshape(n)
        if out is not None and _is_device_tensor(out):
            import torch

            if out.dtype != torch.int32:
                raise ValueError(f"out must be int32, got {out.dtype}")
            if out.device.index != self.device:
                raise ValueError(f"out must be on cuda:{self.device}, got {out.device}")
            if tuple(out.shape) != (n, V) or not out.is_contiguous():
                raise ValueError(f"out must hold ({n}, {V}) contiguous entries")
            dist, ptr, on_dev = out, out.data_ptr(), 1
            torch.cuda.current_stream(out.device).synchronize()   # the library works on its own stream
        elif out is not None:
            raise ValueError("out must be an int32 device tensor")
        else:
            dist = np.empty((n, V), dtype=np.int32)
            ptr, on_dev = dist.ctypes.data, 0
        summ = _lib.LpaSpSummary()
        _lib.check(self._lib.lpa_shortest_paths(self._handle(), lm.ctypes.data_as(_lib._i32p), n, ptr, on_dev,
                                                ctypes.byref(summ) if stats else None))
        return (dist, summ.to_dict()) if stats else dist

    # -- betweenness centrality -----------------------------------------------------
    def betweenness(self, sources=None, directed: bool = True, batch: int = 0, out=None, stats: bool = False):
        """Unscaled betweenness centrality from ``sources`` (distinct dense ids; ``None``: every
        vertex) by Brandes' algorithm (lpa_betweenness): ``raw[v]`` is the sum over the sources
        s != v of the dependency of s on v, over the distinct non-loop arcs of the input graph
        (``directed=False``: every arc in both directions).  With every vertex a source, ``raw``
        (directed) and ``raw / 2`` (undirected) are ``networkx.betweenness_centrality(...,
        normalized=False)``; ``GraphFrame.betweennessCentrality`` applies the scales.  The
        sources run ``batch`` to a pass (1, 4, 8 or 16; 0: the handle's, ``LPA_BC_BATCH`` when
        the handle is created).  Path counts are binary64, as in networkx: above 2^53 they are
        rounded, the result is still deterministic.  Host float64 array of ``num_vertices``
        entries by default, or written into the float64 device tensor ``out`` (this handle's
        device).  ``stats=True`` returns ``(raw, summary)``: ``summary`` is a dict of arcs,
        sources, batches, batch_width, reached, max_depth, levels.  ``raw`` is bit-identical
        across runs, handles, input edge orders and batch widths.  The labels and the LPA state
        are not touched."""
        if not isinstance(batch, (int, np.integer)) or isinstance(batch, (bool, np.bool_)):
            raise TypeError(f"batch must be an int, got {type(batch).__name__}")
        if int(batch) not in (0, 1, 4, 8, 16):
            raise ValueError(f"batch must be 0, 1, 4, 8 or 16, got {int(batch)}")
        V = self.num_vertices
        sv = None
        if sources is not None:
            srcs = list(sources) if not isinstance(sources, (str, bytes)) else [sources]
            for x in srcs:
                if not isinstance(x, (int, np.integer)) or isinstance(x, (bool, np.bool_)):
                    raise TypeError(f"a source must be a dense vertex id (int), got {type(x).__name__}")
            for x in srcs:
                if not 0 <= int(x) < V:
                    raise ValueError(f"source {int(x)} is not a vertex of [0, {V})")
            if len(set(int(x) for x in srcs)) != len(srcs):
                raise ValueError("a source is repeated")
            sv = np.asarray(srcs, dtype=np.int32).reshape(len(srcs))
        if out is not None and _is_device_tensor(out):
            import torch

            if out.dtype != torch.float64:
                raise ValueError(f"out must be float64, got {out.dtype}")
            if out.device.index != self.device:
                raise ValueError(f"out must be on cuda:{self.device}, got {out.device}")
            if out.numel() != V or not out.is_contiguous():
                raise ValueError(f"out must hold {V} contiguous entries")
            raw, ptr, on_dev = out, out.data_ptr(), 1
            torch.cuda.current_stream(out.device).synchronize()   # the library works on its own stream
        elif out is not None:
            raise ValueError("out must be a float64 device tensor")
        else:
            raw = np.empty(V, dtype=np.float64)
            ptr, on_dev = raw.ctypes.data, 0
        summ = _lib.LpaBcSummary()
        _lib.check(self._lib.lpa_betweenness(self._handle(), None if sv is None else sv.ctypes.data_as(_lib._i32p),
                                             0 if sv is None else int(sv.size), 1 if directed else 0, int(batch),
                                             ptr, on_dev, ctypes.byref(summ) if stats else None))
        return (raw, summ.to_dict()) if stats else raw

    # -- breadth-first search ---------------------------------------------------------
    @staticmethod
    def _mask(name, x, n):
        """A boolean or uint8 array of length n as contiguous uint8 (TypeError for another dtype or
        dimension, ValueError for another length)."""
        a = np.asarray(x)
        if a.dtype != np.bool_ and a.dtype != np.uint8:
            raise TypeError(f"{name} must be a boolean or uint8 array, got dtype {a.dtype}")
        if a.ndim != 1:
            raise TypeError(f"{name} must be one-dimensional, got {a.ndim} dimensions")
        if a.size != n:
            raise ValueError(f"{name} must have {n} entries, got {a.size}")
        return np.ascontiguousarray(a).view(np.uint8)

    def bfs(self, from_mask, to_mask, edge_keep=None, max_path_length: int = 10, stats: bool = False):
        """Breadth-first search between two vertex sets of the directed input graph (lpa_bfs;
        GraphFrames ``lib.BFS``): F = the vertices of ``from_mask``, T = those of ``to_mask``
        (boolean or uint8 arrays of ``num_vertices`` entries), over the input edges that
        ``edge_keep`` (``num_edges`` entries, ``None``: all) keeps, self-loops never.  Returns
        ``(length, level, edge_index)``: ``length`` is the fewest edges on a path from F to T, 0
        when the sets share a vertex, -1 when there is no path of at most ``max_path_length``
        edges (or a set is empty); ``level`` (int32, ``num_vertices`` entries) is the place of a
        vertex on a path of ``length`` edges from F to T and -1 off all of them; ``edge_index``
        (int64, ascending) lists the input edges on such a path, a duplicate edge beside its
        twin.  Every path of ``length`` edges from F to T is a walk over those edges from level
        0 to level ``length`` (``enumerate_paths`` lists them).  ``stats=True`` adds ``summary``,
        a dict of arcs, sources, targets, length, reached, path_vertices, path_edges,
        push_levels, pull_levels.  The result is identical across runs, handles and push / pull
        schedules, ``level`` across input edge orders too.  The labels and the LPA state are not
        touched."""
        if not isinstance(max_path_length, (int, np.integer)) or isinstance(max_path_length, (bool, np.bool_)):
            raise TypeError(f"max_path_length must be an int, got {type(max_path_length).__name__}")
        if max_path_length < 0:
            raise ValueError(f"max_path_length must not be negative, got {max_path_length}")
        V, m = self.num_vertices, self.num_edges
        fm = self._mask("from_mask", from_mask, V)
        tm = self._mask("to_mask", to_mask, V)
        keep = None if edge_keep is None else self._mask("edge_keep", edge_keep, m)
        level = np.empty(V, dtype=np.int32)
        on_edge = np.empty(m, dtype=np.uint8)
        summ = _lib.LpaBfsSummary()
        u8 = _lib._u8p
        _lib.check(self._lib.lpa_bfs(self._handle(), fm.ctypes.data_as(u8), tm.ctypes.data_as(u8),
                                     None if keep is None else keep.ctypes.data_as(u8),
                                     min(int(max_path_length), 2 ** 31 - 1), level.ctypes.data_as(_lib._i32p),
                                     on_edge.ctypes.data_as(u8), ctypes.byref(summ)))
        res = (int(summ.length), level, np.flatnonzero(on_edge.view(np.bool_)).astype(np.int64, copy=False))
        return res + (summ.to_dict(),) if stats else res

    # -- motif finding ----------------------------------------------------------------
    def motif(self, n_vars: int, terms, var_out=None, max_rows=None, count_only: bool = False, stats: bool = False):
        """Motif finding over the directed input multigraph (lpa_motif; GraphFrames
        ``GraphFrame.find``) for a parsed pattern: ``n_vars`` vertex variables and ``terms``, a
        sequence of ``(src_var, dst_var, negated, want_edge)`` run in that order.  The first term
        is positive; a later positive term shares a variable with the ones before it; a negated
        term reads bound variables only.  A row is one assignment of vertices to the bound
        variables and of input edge rows to the positive terms: duplicate edges multiply rows,
        variables need not differ, self-loops are edges.  ``var_out`` lists the variables whose
        columns are wanted (``None``: every bound one).  Returns ``(vertex_cols, edge_cols)``:
        ``vertex_cols[var]`` int32 dense ids, ``edge_cols[term]`` int64 input edge rows for the
        terms with ``want_edge``, all of one length, in the library's deterministic row order;
        with ``count_only`` the exact row count alone, nothing materialised.  ``max_rows``
        (``None`` or <= 0: no cap) bounds every table, intermediate or final: a step that needs
        more raises ``ValueError`` naming the step and the rows it needed.  ``stats=True`` adds
        ``summary``, a dict of rows, edges, self_loops, steps, peak_rows, overflow_step,
        overflow_rows, table_rows.  The labels and the LPA state are not touched."""
        tl = [tuple(int(x) for x in t) for t in terms]
        if any(len(t) != 4 for t in tl):
            raise ValueError("a motif term is (src_var, dst_var, negated, want_edge)")
        n_vars = int(n_vars)
        arr = (_lib.LpaMotifTerm * max(len(tl), 1))()
        bound = set()
        for i, (a, b, neg, we) in enumerate(tl):
            arr[i] = _lib.LpaMotifTerm(a, b, neg, we)
            if not neg:
                bound.update((a, b))
        if var_out is None:
            var_out = sorted(v for v in bound if 0 <= v < n_vars)
        var_out = [int(v) for v in var_out]
        if any(v < 0 or v >= n_vars for v in var_out):
            raise ValueError(f"var_out names a variable outside [0, {n_vars})")
        mask = np.zeros(max(n_vars, 1), dtype=np.uint8)
        mask[var_out] = 1
        cap = 0 if max_rows is None else int(max_rows)
        summ = _lib.LpaMotifSummary()
        res = ctypes.c_void_p()
        lib = self._lib
        try:
            rc = lib.lpa_motif(self._handle(), n_vars, mask.ctypes.data_as(_lib._u8p), arr, len(tl), cap,
                               1 if count_only else 0, None if count_only else ctypes.byref(res), ctypes.byref(summ))
            if rc == _lib.LPA_EOVERFLOW and summ.overflow_step >= 0:
                raise ValueError(f"motif: step {summ.overflow_step} needs {summ.overflow_rows} rows, "
                                 f"more than max_rows = {cap}")
            _lib.check(rc)
            if count_only:
                out = int(summ.rows)
                return (out, summ.to_dict()) if stats else out
            rows = int(lib.lpa_motif_rows(res))
            vcols, ecols = {}, {}
            for v in var_out:
                col = np.empty(rows, dtype=np.int32)
                _lib.check(lib.lpa_motif_vertex_column(res, v, col.ctypes.data_as(_lib._i32p)))
                vcols[v] = col
            for i, (_, _, neg, we) in enumerate(tl):
                if we and not neg:
                    col = np.empty(rows, dtype=np.int64)
                    _lib.check(lib.lpa_motif_edge_column(res, i, col.ctypes.data_as(_lib._i64p)))
                    ecols[i] = col
            return (vcols, ecols, summ.to_dict()) if stats else (vcols, ecols)
        finally:
            lib.lpa_motif_result_destroy(res)

    # -- message aggregation ----------------------------------------------------------
    @staticmethod
    def _program_array(progs, struct, what):
        """Compiled programs (``ops``, ``consts``) as one C array of the ABI's fixed-size struct."""
        progs = list(progs)
        arr = (struct * max(len(progs), 1))()
        for k, prog in enumerate(progs):
            ops, consts = list(prog.ops), list(prog.consts)
            if len(ops) > _lib.LPA_AM_MAX_OPS or len(consts) > _lib.LPA_AM_MAX_CONSTS:
                raise ValueError(f"a {what} program holds at most {_lib.LPA_AM_MAX_OPS} ops and "
                                 f"{_lib.LPA_AM_MAX_CONSTS} constants, got {len(ops)} and {len(consts)}")
            arr[k].n_ops, arr[k].n_consts = len(ops), len(consts)
            for i, (op, arg) in enumerate(ops):
                if not 0 <= int(op) <= 0xFFFF or not 0 <= int(arg) <= 0xFFFF:
                    raise ValueError(f"op {i}: opcode and argument are 16-bit values, got {op} and {arg}")
                arr[k].ops[i] = int(op) | (int(arg) << 16)
            for i, c in enumerate(consts):
                arr[k].consts[i] = float(c)
        return arr, len(progs)

    @staticmethod
    def _am_program(prog):
        """A compiled message (``ops``: (opcode, argument) pairs, ``consts``: floats) as the C ABI's
        fixed-size struct; ``None`` stays ``None``."""
        return None if prog is None else Graph._program_array([prog], _lib.LpaAmProgram, "message")[0][0]

    def aggregate_messages(self, to_src, to_dst, vcols=None, ecols=None, stats: bool = False):
        """Message aggregation over the directed input multigraph (lpa_aggregate_messages;
        GraphFrames ``aggregateMessages``): every input edge evaluates the compiled message
        ``to_dst`` for its destination and ``to_src`` for its source (``compile_message``
        results or ``None``, not both ``None``), every vertex reduces what it receives.
        ``vcols`` is ``[n_vcols, num_vertices]`` float64, ``ecols`` ``[n_ecols, num_edges]``
        float64 in the handle's input edge order (``None``: no columns).  Returns a dict of
        ``num_vertices``-entry arrays: ``count`` (int64), ``sum`` (0.0 where count is 0),
        ``min`` and ``max`` (NaN where count is 0); with ``stats=True`` ``(dict, summary)``,
        the summary a dict of edges, messages_to_src, messages_to_dst, nulls, receivers,
        rows_short, rows_wave, rows_block, max_row.  Duplicate edges send again; a null
        message is not delivered.  ``count``, ``min`` and ``max`` depend on the inputs alone;
        ``sum`` is bit-identical across calls and handles, and across input edge orders for a
        program that reads no edge column.  The labels and the LPA state are not touched."""
        V, m = self.num_vertices, self.num_edges

        def cols(x, n, name):
            if x is None:
                return np.empty((0, n), dtype=np.float64)
            a = np.ascontiguousarray(x, dtype=np.float64)
            if a.ndim != 2 or a.shape[1] != n:
                raise ValueError(f"{name} must have the shape [columns, {n}], got {list(a.shape)}")
            return a

        vc, ec = cols(vcols, V, "vcols"), cols(ecols, m, "ecols")
        ps, pd_ = self._am_program(to_src), self._am_program(to_dst)
        out = dict(count=np.empty(V, dtype=np.int64), sum=np.empty(V, dtype=np.float64),
                   min=np.empty(V, dtype=np.float64), max=np.empty(V, dtype=np.float64))
        summ = _lib.LpaAmSummary()
        _lib.check(self._lib.lpa_aggregate_messages(
            self._handle(), None if ps is None else ctypes.byref(ps), None if pd_ is None else ctypes.byref(pd_),
            vc.ctypes.data if vc.shape[0] else None, vc.shape[0], ec.ctypes.data if ec.shape[0] else None,
            ec.shape[0], out["count"].ctypes.data, out["sum"].ctypes.data, out["min"].ctypes.data,
            out["max"].ctypes.data, ctypes.byref(summ) if stats else None))
        return (out, summ.to_dict()) if stats else out

    # -- Pregel -----------------------------------------------------------------------
    def pregel(self, max_iter, agg, to_src, to_dst, init, update, vcols=None, ecols=None, stats: bool = False):
        """Pregel over the directed input multigraph (lpa_pregel; ``graphframes.lib.Pregel``):
        ``len(init) == len(update)`` Pregel columns (1 to 4) live on the device for ``max_iter``
        iterations.  Column j starts as the vertex program ``init[j]``; an iteration evaluates
        the compiled messages ``to_dst`` (for the destination) and ``to_src`` (for the source)
        of every input edge (lists of ``compile_message`` results, 0 to 4 each, not both empty),
        reduces what a vertex receives with ``agg`` (``"sum"``, ``"min"``, ``"max"``, ``"avg"``,
        ``"count"``) to ``msg`` -- null where nothing arrived -- and sets column j to
        ``update[j]`` (``compile_vertex_program`` results) over the vertex's old columns and
        ``msg``, all columns at once.  Column indices: the static columns ``vcols``
        (``[n_vcols, num_vertices]`` float64) come first, then the Pregel columns; ``ecols`` is
        ``[n_ecols, num_edges]`` float64 in the handle's input edge order.  Returns the columns
        after ``max_iter`` iterations, ``[n_pcols, num_vertices]`` float64; with ``stats=True``
        ``(columns, summary)``, the summary a dict of edges, messages_to_src, messages_to_dst,
        nulls (all three summed over the iterations), rows_short, rows_wave, rows_block, max_row,
        iterations.  A null initial or updated value raises ``PregelNullError`` (a
        ``ValueError`` with ``iteration`` -- 0 for the start --, ``column`` and ``vertex``).
        With min, max or count the columns depend on the inputs alone; with sum or avg they are
        bit-identical across calls and handles, and across input edge orders for programs that
        read no edge column.  The labels and the LPA state are not touched."""
        V, m = self.num_vertices, self.num_edges
        if agg not in _lib.PG_AGGREGATES:
            raise ValueError(f"agg must be one of {', '.join(_lib.PG_AGGREGATES)}, got {agg!r}")

        def cols(x, n, name):
            if x is None:
                return np.empty((0, n), dtype=np.float64)
            a = np.ascontiguousarray(x, dtype=np.float64)
            if a.ndim != 2 or a.shape[1] != n:
                raise ValueError(f"{name} must have the shape [columns, {n}], got {list(a.shape)}")
            return a

        vc, ec = cols(vcols, V, "vcols"), cols(ecols, m, "ecols")
        if len(init) != len(update):
            raise ValueError(f"init and update hold one program per Pregel column, got {len(init)} and {len(update)}")
        ps, n_ps = self._program_array(to_src or (), _lib.LpaAmProgram, "message")
        pd_, n_pd = self._program_array(to_dst or (), _lib.LpaAmProgram, "message")
        pi, n_p = self._program_array(init, _lib.LpaVpProgram, "vertex")
        pu, _ = self._program_array(update, _lib.LpaVpProgram, "vertex")
        out = np.empty((n_p, V), dtype=np.float64)
        summ = _lib.LpaPregelSummary()
        summ.null_iteration = -1   # set by the call only once the arguments have passed
        rc = self._lib.lpa_pregel(self._handle(), int(max_iter), _lib.PG_AGGREGATES.index(agg), ps, n_ps, pd_, n_pd,
                                  pi, pu, n_p, vc.ctypes.data if vc.shape[0] else None, vc.shape[0],
                                  ec.ctypes.data if ec.shape[0] else None, ec.shape[0], out.ctypes.data,
                                  ctypes.byref(summ))
        if rc == _lib.LPA_EINVAL and summ.null_iteration >= 0:
            raise PregelNullError(_lib.last_error(), int(summ.null_iteration), int(summ.null_column),
                                  int(summ.null_vertex))
        _lib.check(rc)
        return (out, summ.to_dict()) if stats else out

    # -- strongly connected components ------------------------------------------------
    def strongly_connected_components(self, max_iter=None, out=None, sizes: bool = False):
        """Strongly connected components of the directed input graph
        (lpa_strongly_connected_components; GraphX ``lib.StronglyConnectedComponents``): at most
        ``max_iter`` rounds of trim, forward colouring and backward sweep; ``None`` runs to
        convergence.  Converged, ``comp[v]`` is the smallest dense id of v's SCC; stopped early,
        a vertex whose SCC has not been written yet holds its own id (``max_iter=1`` gives the
        identity), exactly as GraphX.  Duplicate edges change nothing; a self-loop changes only
        the round in which its vertex leaves.  Host int32 array by default, or written into the
        int32 device tensor ``out`` (this handle's device, ``num_vertices`` entries).
        ``sizes=True`` returns ``(comp, sizes, summary)``: ``sizes[c]`` (int64, in the memory
        ``comp`` is in) holds the member count at every component id c and 0 elsewhere;
        ``summary`` is a dict of n_components, n_singletons, largest_size, largest_id, rounds,
        trimmed, unresolved (0 exactly when converged).  The result is identical across runs,
        handles, input edge orders and kernel schedules.  The labels and the LPA state are not
        touched."""
        if max_iter is None:
            max_iter = 2 ** 31 - 1
        if not isinstance(max_iter, (int, np.integer)) or isinstance(max_iter, (bool, np.bool_)):
            raise TypeError(f"max_iter must be an int or None, got {type(max_iter).__name__}")
        if max_iter <= 0:
            raise ValueError(f"max_iter must be greater than 0, got {max_iter}")
        max_iter = min(int(max_iter), 2 ** 31 - 1)
        V = self.num_vertices
        size = None
        if out is not None and _is_device_tensor(out):
            import torch

            if out.dtype != torch.int32:
                raise ValueError(f"out must be int32, got {out.dtype}")
            if out.device.index != self.device:
                raise ValueError(f"out must be on cuda:{self.device}, got {out.device}")
            if out.numel() != V or not out.is_contiguous():
                raise ValueError(f"out must hold {V} contiguous entries")
            comp, ptr, on_dev = out, out.data_ptr(), 1
            if sizes:
                size = torch.empty(V, dtype=torch.int64, device=out.device)
            torch.cuda.current_stream(out.device).synchronize()   # the library works on its own stream
            size_ptr = size.data_ptr() if sizes else None
        elif out is not None:
            raise ValueError("out must be an int32 device tensor")
        else:
            comp = np.empty(V, dtype=np.int32)
            ptr, on_dev = comp.ctypes.data, 0
            if sizes:
                size = np.empty(V, dtype=np.int64)
            size_ptr = size.ctypes.data if sizes else None
        summ = _lib.LpaSccSummary()
        _lib.check(self._lib.lpa_strongly_connected_components(self._handle(), max_iter, ptr, on_dev, size_ptr,
                                                               ctypes.byref(summ) if sizes else None))
        return (comp, size, summ.to_dict()) if sizes else comp

    # -- Louvain ------------------------------------------------------------------------
    def louvain(self, max_levels: int = 64, max_rounds: int = 1000, out=None, stats: bool = False):
        """Louvain community detection on the symmetrised multigraph the labels are voted on
        and ``quality`` scores (lpa_louvain): a synchronous, deterministic Louvain in exact
        integer arithmetic -- every round each vertex proposes its best neighbouring community
        by the modularity gain (ties to the smaller id, two singletons merge towards the
        smaller id), all proposals are applied if the modularity rises, otherwise only those to
        a smaller id, otherwise the level ends; the communities then become the vertices of the
        next level, at most ``max_levels`` levels of at most ``max_rounds`` rounds each.
        ``comm[v]`` is the smallest dense id of v's community.  A path or a cycle of n vertices
        is the slow case, about n / 2 rounds in the first level: ``max_rounds`` is the bound.
        Host int32 array by default, or written into the int32 device tensor ``out`` (this
        handle's device, ``num_vertices`` entries).  ``stats=True`` returns ``(comm, sizes,
        levels, summary)``: ``sizes[c]`` (int64, in the memory ``comm`` is in) holds the member
        count at every community id c and 0 elsewhere; ``levels`` is a list of dicts of
        vertices, communities, rounds, damped_rounds, moves, numerator, one per level;
        ``summary`` a dict of n_communities, n_singletons, largest_size, largest_id, levels,
        rounds, damped_rounds, moves, arcs, intra_arcs, numerator, modularity.  The result is
        identical across runs, handles, input edge orders and directions, and kernel
        schedules.  The labels and the LPA state are not touched."""
        for name, x in (("max_levels", max_levels), ("max_rounds", max_rounds)):
            if not isinstance(x, (int, np.integer)) or isinstance(x, (bool, np.bool_)):
                raise TypeError(f"{name} must be an int, got {type(x).__name__}")
            if x <= 0:
                raise ValueError(f"{name} must be greater than 0, got {x}")
        max_levels = min(int(max_levels), 2 ** 31 - 1)
        max_rounds = min(int(max_rounds), 2 ** 31 - 1)
        V = self.num_vertices
        size = None
        if out is not None and _is_device_tensor(out):
            import torch

            if out.dtype != torch.int32:
                raise ValueError(f"out must be int32, got {out.dtype}")
            if out.device.index != self.device:
                raise ValueError(f"out must be on cuda:{self.device}, got {out.device}")
            if out.numel() != V or not out.is_contiguous():
                raise ValueError(f"out must hold {V} contiguous entries")
            comm, ptr, on_dev = out, out.data_ptr(), 1
            if stats:
                size = torch.empty(V, dtype=torch.int64, device=out.device)
            torch.cuda.current_stream(out.device).synchronize()   # the library works on its own stream
            size_ptr = size.data_ptr() if stats else None
        elif out is not None:
            raise ValueError("out must be an int32 device tensor")
        else:
            comm = np.empty(V, dtype=np.int32)
            ptr, on_dev = comm.ctypes.data, 0
            if stats:
                size = np.empty(V, dtype=np.int64)
            size_ptr = size.ctypes.data if stats else None
        cap = min(max_levels, 1024)   # level rows returned; later levels (unseen so far) count in the summary only
        rows = (_lib.LpaLouvainLevel * cap)()
        summ = _lib.LpaLouvainSummary()
        _lib.check(self._lib.lpa_louvain(self._handle(), max_levels, max_rounds, ptr, on_dev, size_ptr,
                                         rows if stats else None, cap if stats else 0,
                                         ctypes.byref(summ) if stats else None))
        if not stats:
            return comm
        return comm, size, [rows[i].to_dict() for i in range(min(int(summ.levels), cap))], summ.to_dict()

    # -- k-core decomposition -----------------------------------------------------------
    def core_numbers(self, max_k=None, out=None, stats: bool = False):
        """Core numbers of the canonical simple undirected graph of the input multigraph
        (lpa_core_numbers: self-loops dropped, direction ignored, duplicates collapsed, as
        ``triangle_count``): ``core[v]`` is the largest k such that v lies in a subgraph where
        every vertex has at least k neighbours; 0 for a vertex without a neighbour.  ``max_k``
        (an int >= 0, ``None``: no cap) gives ``min(core, max_k)`` and stops the peeling before
        level ``max_k``; ``max_k=0`` only builds the graph.  Host int32 array by default, or
        written into the int32 device tensor ``out`` (this handle's device, ``num_vertices``
        entries).  ``stats=True`` returns ``(core, simple_degree, summary)``:
        ``simple_degree[v]`` (int32, in the memory ``core`` is in) is the number of distinct
        neighbours of v; ``summary`` is a dict of degeneracy, main_core_size (both of the capped
        values), levels, simple_edges, max_degree, n_core0 and passes (the peel's host round
        trips: the schedule, not a property of the graph).  The result is identical across
        runs, handles, input edge orders and directions, and kernel schedules.  The labels and
        the LPA state are not touched."""
        if max_k is None:
            max_k = 2 ** 31 - 1
        if not isinstance(max_k, (int, np.integer)) or isinstance(max_k, (bool, np.bool_)):
            raise TypeError(f"max_k must be an int or None, got {type(max_k).__name__}")
        if max_k < 0:
            raise ValueError(f"max_k must not be negative, got {max_k}")
        max_k = min(int(max_k), 2 ** 31 - 1)
        V = self.num_vertices
        deg = None
        if out is not None and _is_device_tensor(out):
            import torch

            if out.dtype != torch.int32:
                raise ValueError(f"out must be int32, got {out.dtype}")
            if out.device.index != self.device:
                raise ValueError(f"out must be on cuda:{self.device}, got {out.device}")
            if out.numel() != V or not out.is_contiguous():
                raise ValueError(f"out must hold {V} contiguous entries")
            core, ptr, on_dev = out, out.data_ptr(), 1
            if stats:
                deg = torch.empty(V, dtype=torch.int32, device=out.device)
            torch.cuda.current_stream(out.device).synchronize()   # the library works on its own stream
            deg_ptr = deg.data_ptr() if stats else None
        elif out is not None:
            raise ValueError("out must be an int32 device tensor")
        else:
            core = np.empty(V, dtype=np.int32)
            ptr, on_dev = core.ctypes.data, 0
            if stats:
                deg = np.empty(V, dtype=np.int32)
            deg_ptr = deg.ctypes.data if stats else None
        summ = _lib.LpaCoreSummary()
        _lib.check(self._lib.lpa_core_numbers(self._handle(), max_k, ptr, deg_ptr, on_dev,
                                              ctypes.byref(summ) if stats else None))
        return (core, deg, summ.to_dict()) if stats else core

    # -- SCAN structural clustering -----------------------------------------------------
    def scan(self, eps, mu, out=None, stats: bool = False, common: bool = False):
        """SCAN structural clustering (Xu et al., KDD 2007; lpa_scan, include/lpa.h states the
        definition) of the canonical simple undirected graph of the input multigraph (self-loops
        dropped, direction ignored, duplicates collapsed, as ``triangle_count``).  An edge
        {u, v} with c common neighbours is similar iff ``(c+2)^2 >= eps^2 (d[u]+1) (d[v]+1)`` in
        binary64; a vertex with ``nsim + 1 >= mu`` similar edges (itself counted) is a core;
        cores joined over similar edges form a cluster, labelled by its smallest core; a
        non-core with a similar edge to a core is a border of the smallest such label; every
        other vertex keeps its own id as label and is a hub (its neighbours carry at least two
        cluster labels) or an outlier.  ``eps`` in (0, 1], ``mu`` an int >= 1.
        Returns ``(label, role)``: int32 labels (dense ids) and uint8 roles (0 outlier, 1 hub,
        2 border, 3 core; ``SCAN_ROLES`` names them), host arrays by default, or with ``label``
        written into the int32 device tensor ``out`` (this handle's device, ``num_vertices``
        entries) and every other array a device tensor beside it.  ``stats=True`` appends
        ``nsim`` (int32: similar edges per vertex) and ``summary`` (a dict of simple_edges,
        triangles, similar_edges, n_clusters, n_cores, n_borders, n_hubs, n_outliers,
        largest_cluster, largest_cluster_label).  ``common=True`` appends, last, ``common``
        (int32, one entry per input edge row): the common neighbours of the row's edge, -1 for
        a self-loop row or one with an end outside the vertex range.  The result is a function
        of the vertex count, the edge set, eps and mu alone.  The labels and the LPA state are
        not touched."""
        eps, mu = _check_scan(eps, mu)
        V, m = self.num_vertices, self.num_edges
        nsim = cmn = None
        if out is not None and _is_device_tensor(out):
            import torch

            if out.dtype != torch.int32:
                raise ValueError(f"out must be int32, got {out.dtype}")
            if out.device.index != self.device:
                raise ValueError(f"out must be on cuda:{self.device}, got {out.device}")
            if out.numel() != V or not out.is_contiguous():
                raise ValueError(f"out must hold {V} contiguous entries")
            label, on_dev = out, 1
            role = torch.empty(V, dtype=torch.uint8, device=out.device)
            if stats:
                nsim = torch.empty(V, dtype=torch.int32, device=out.device)
            if common:
                cmn = torch.empty(m, dtype=torch.int32, device=out.device)
            torch.cuda.current_stream(out.device).synchronize()   # the library works on its own stream
            ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
        elif out is not None:
            raise ValueError("out must be an int32 device tensor")
        else:
            label, on_dev = np.empty(V, dtype=np.int32), 0
            role = np.empty(V, dtype=np.uint8)
            if stats:
                nsim = np.empty(V, dtype=np.int32)
            if common:
                cmn = np.empty(m, dtype=np.int32)
            ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        summ = _lib.LpaScanSummary()
        _lib.check(self._lib.lpa_scan(self._handle(), eps, mu, ptr(label), ptr(role), ptr(nsim), ptr(cmn), on_dev,
                                      ctypes.byref(summ) if stats else None))
        res = (label, role) + ((nsim, summ.to_dict()) if stats else ()) + ((cmn,) if common else ())
        return res


class Loopback:
    """In-process collective group of ``nranks`` handles on one device (the
    multi-GPU exchange rehearsed on one GPU).  Drive each rank's Graph from its own
    thread; ctypes releases the GIL during the library calls."""

    def __init__(self, nranks: int):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.lpa_loopback_create(int(nranks), ctypes.byref(self._h)))
        self.nranks = int(nranks)

    def _handle(self):
        if not self._h:
            raise ValueError("loopback group is closed")
        return self._h

    def abort(self):
        """Release every thread blocked in a collective of this group (they fail)."""
        if self._h:
            self._lib.lpa_loopback_abort(self._h)

    def close(self):
        if self._h:
            self._lib.lpa_loopback_destroy(self._h)
            self._h = ctypes.c_void_p()


def run_ranks(graphs, fn):
    """Call ``fn(rank, graph)`` for every rank of a loopback group on its own thread;
    returns the results in rank order, re-raising the first failure in time (after
    aborting the group so no thread stays blocked in a collective)."""
    import threading

    res = [None] * len(graphs)
    errs = []   # in the order the ranks failed: the first is the cause, the rest
    lock = threading.Lock()   # are peers released by the abort

    def work(r):
        try:
            res[r] = fn(r, graphs[r])
        except BaseException as e:  # noqa: BLE001 -- re-raised below
            with lock:
                errs.append(e)
            lb = graphs[r]._loopback
            if lb is not None:
                lb.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(len(graphs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0]
    return res


def comm_unique_id() -> bytes:
    """RCCL unique id for a distributed build (create on one rank, broadcast)."""
    buf = ctypes.create_string_buffer(128)
    _lib.check(_lib.load().lpa_comm_unique_id(buf))
    return buf.raw


def gen_rmat(scale: int, edgefactor: int = 16, seed: int = 1, scramble: bool = True, device: int = 0):
    """R-MAT edge list generated in HBM (torch int32 tensors on `device`)."""
    import torch

    m = edgefactor << scale
    dev = torch.device("cuda", device)
    src = torch.empty(m, dtype=torch.int32, device=dev)
    dst = torch.empty(m, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    _lib.check(_lib.load().lpa_gen_rmat(scale, m, seed, int(scramble), src.data_ptr(), dst.data_ptr(),
                                        device, None))
    return src, dst


def gen_sbm(num_vertices: int, blocks: int, m: int, seed: int = 20261015,
            p_in_q32: int = 3865470566, device: int = 0):
    """Planted-partition SBM edge list generated in HBM (p_in = p_in_q32 / 2^32)."""
    import torch

    dev = torch.device("cuda", device)
    src = torch.empty(m, dtype=torch.int32, device=dev)
    dst = torch.empty(m, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    _lib.check(_lib.load().lpa_gen_sbm(num_vertices, blocks, m, p_in_q32, seed, src.data_ptr(),
                                       dst.data_ptr(), device, None))
    return src, dst


def gen_chunglu(num_vertices: int, m: int, gamma: float = 2.1, max_deg: float = 0.0, seed: int = 7,
                device: int = 0):
    """Chung-Lu power-law edge list generated in HBM (config C5: heavy hubs)."""
    import torch

    dev = torch.device("cuda", device)
    src = torch.empty(m, dtype=torch.int32, device=dev)
    dst = torch.empty(m, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    _lib.check(_lib.load().lpa_gen_chunglu(num_vertices, m, gamma, max_deg, seed, src.data_ptr(),
                                           dst.data_ptr(), device, None))
    return src, dst
