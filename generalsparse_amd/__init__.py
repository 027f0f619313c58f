"""generalsparse_amd -- MI355X-native SpMM (C = sparse_A x dense_B) behind
GeneralSparse's operator / plan surface.

Host-side mirror of the reference interface, over the C ABI of
libgeneralsparse.so (include/generalsparse.h):

    plan = Plan.from_mtx("m.mtx")                  # create_init_metadata_set_from_file
    plan.add_operator("sort_operator")              # operator_executer::add_and_run
    plan.add_operator("fixed_interval_row_direction_thread_blocking_operator",
                      1, 0, 0, 0, 0, 1, 4)
    plan.add_operator("thread_total_reduce_operator", 0, 4, 1)
    plan.compile()                                  # code_generator::compile
    plan.upload(dtype="f16")                        # or "f32" / "bf16" (A's values, B and C)
    C = plan.spmm(B)                                # the generated kernel, on the GPU

or the canned token_test pipelines: plan.run_pipeline("warp_segment", N=32).
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import GS_BF16, GS_F16, GS_F32, GS_W_FP8_E4M3, GS_W_NATIVE, GsError

__all__ = ["Plan", "Batch", "LinearBatch", "Rotation", "SparseLinear", "SparseLinearGroup", "set_config", "GsError", "GS_F16", "GS_F32", "GS_BF16", "PIPELINES", "load_library",
           "convert_values", "GS_W_NATIVE", "GS_W_FP8_E4M3", "fp8_quantize", "fp8_decode", "sddmm_geometry"]

# token_test.cc pipelines (+ the two compositions this engine adds)
PIPELINES = ("thread_total", "warp_total", "block_total", "thread_bit_map", "warp_segment",
             "tblock_warp_total", "balanced_warp_total", "warp_bit_map", "tblock_bit_map", "col_direction_nm")


def load_library():
    return _lib.load()


def set_config(key, value):
    """set_config (config.cc:17-40); process-wide, in memory."""
    L = _lib.load()
    _lib.check(L.gs_set_config_int(key.encode(), int(value)))


def get_config(key):
    """the current value of an integer / bool config key"""
    L = _lib.load()
    v = ctypes.c_longlong()
    _lib.check(L.gs_get_config_int(key.encode(), ctypes.byref(v)))
    return v.value


def _dtype_code(dtype):
    if dtype in (GS_F16, "f16", "fp16", "half", np.float16):
        return GS_F16
    if dtype in (GS_F32, "f32", "fp32", "float", np.float32):
        return GS_F32
    if dtype in (GS_BF16, "bf16", "bfloat16"):
        return GS_BF16
    try:
        import torch
        if dtype == torch.float16:
            return GS_F16
        if dtype == torch.float32:
            return GS_F32
        if dtype == torch.bfloat16:
            return GS_BF16
    except ImportError:
        pass
    raise ValueError(f"unsupported dtype {dtype}")


def convert_values(values, dtype):
    """fp32 values in a plan dtype's storage type, as upload() stores A's values
    (gs_convert_values: round to nearest even): a float32 array for "f32", the 16-bit words as a
    uint16 array for "f16" / "bf16" (numpy has no bfloat16)"""
    L = _lib.load()
    code = _dtype_code(dtype)
    x = np.ascontiguousarray(values, dtype=np.float32).ravel()
    out = np.empty(x.size, np.float32 if code == GS_F32 else np.uint16)
    _lib.check(L.gs_convert_values(x.ctypes.data_as(_lib.f32p), x.size, code, ctypes.c_void_p(out.ctypes.data)))
    return out


def _weights_code(weights):
    if weights in (None, GS_W_NATIVE, "native"):
        return GS_W_NATIVE
    if weights in (GS_W_FP8_E4M3, "fp8", "fp8_e4m3", "e4m3"):
        return GS_W_FP8_E4M3
    raise ValueError(f"unsupported weights {weights!r} (None or \"fp8\")")


def fp8_quantize(val, row, n_rows, row_scale=None):
    """A's values as Plan.upload(weights="fp8") stores them (gs_quantize_fp8_rows): (codes, scale) with
    codes[i] = e4m3fn(val[i] / scale[row[i]]) as uint8 -- an IEEE float32 division, rounded to nearest even
    and saturated at +-448 (never a NaN code) -- and scale the n_rows float32 scales used: row_scale, or
    by default 2^e with the smallest e such that max|val of the row| / 2^e <= 448 (1 for a row without
    values).  Refused (GsError): a non-finite value, a row >= n_rows, a scale that is not finite and > 0,
    a row_scale of another length."""
    L = _lib.load()
    v = np.ascontiguousarray(val, dtype=np.float32).ravel()
    r = np.asarray(row).ravel()
    if r.size != v.size:
        raise _refused("fp8_quantize: val and row lengths differ")
    if r.size and (not np.issubdtype(r.dtype, np.integer) or r.min() < 0):
        raise _refused("fp8_quantize: row must hold non-negative integers")
    r = np.ascontiguousarray(r, dtype=np.uint64)
    sp, ns = None, 0
    if row_scale is not None:
        row_scale = np.ascontiguousarray(row_scale, dtype=np.float32).ravel()
        sp, ns = row_scale.ctypes.data_as(_lib.f32p), row_scale.size
    codes = np.zeros(v.size, np.uint8)
    scale = np.zeros(int(n_rows), np.float32)
    _lib.check(L.gs_quantize_fp8_rows(v.ctypes.data_as(_lib.f32p), r.ctypes.data_as(_lib.u64p), v.size, int(n_rows), sp, ns,
                                      codes.ctypes.data_as(_lib.u8p), scale.ctypes.data_as(_lib.f32p)))
    return codes, scale


def fp8_decode(codes):
    """OCP e4m3fn codes (uint8) as float32, exactly (gs_fp8_decode); 0x7f / 0xff give NaN"""
    L = _lib.load()
    c = np.ascontiguousarray(codes, dtype=np.uint8)
    out = np.zeros(c.size, np.float32)
    _lib.check(L.gs_fp8_decode(c.ravel().ctypes.data_as(_lib.u8p), c.size, out.ctypes.data_as(_lib.f32p)))
    return out.reshape(c.shape)


def sddmm_geometry():
    """(row_block, col_strip, token_chunk) of k_sddmm_tm (gs_sddmm_geometry): output features per
    workgroup, input features per wave strip, tokens per chunk"""
    L = _lib.load()
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(L.gs_sddmm_geometry(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


def _torch_dtype(code):
    """the torch dtype of B and C for a plan's dtype code"""
    import torch
    return {GS_F32: torch.float32, GS_F16: torch.float16, GS_BF16: torch.bfloat16}[code]


def index_compression_of_array(a, type_ori=16, branch_max=5):
    """the reference's compression decision for a raw u64 array: (kind, {coef, intercept,
    cycle, aa, bb}, exact); type_ori = the gs data_type code of its storage (16 = u64)"""
    L = _lib.load()
    a = np.ascontiguousarray(a, dtype=np.uint64)
    kind = ctypes.create_string_buffer(32)
    prm = np.zeros(5, np.uint64)
    ex = ctypes.c_int(0)
    _lib.check(L.gs_index_compression_of_array(a.ctypes.data_as(_lib.u64p), len(a), int(type_ori), int(branch_max), kind, 32,
                                               prm.ctypes.data_as(_lib.u64p), ctypes.byref(ex)))
    p = {"coef": int(prm[0]), "intercept": int(prm[1]), "cycle": int(prm[2]),
         "aa": int(prm[3].astype(np.int64)), "bb": int(prm[4].astype(np.int64))}
    return kind.value.decode(), p, bool(ex.value)


def _refused(msg):
    """the error the library raises for a refused argument (GS_ERR code -1)"""
    e = GsError(f"generalsparse error -1: {msg}")
    e.code = -1
    return e


def _check_operands(info, B, C, N=None):
    """B (cols x N) and C (rows x N): contiguous GPU tensors of the plan's dtype on one device.
    The kernels read B and write every row of C at stride N, so a short or strided operand would
    be read or written out of bounds; raw pointers (ints) are the caller's responsibility."""
    want = _torch_dtype(info["dtype"])
    if not (B.is_cuda and B.dim() == 2 and B.is_contiguous()):
        raise ValueError("B must be a contiguous 2-D GPU tensor")
    if B.shape[0] != info["cols"]:
        raise ValueError(f"B has {B.shape[0]} rows, A has {info['cols']} columns")
    if B.dtype != want:
        raise TypeError(f"B must be {want}")
    N = B.shape[1] if N is None else N
    if B.shape[1] != N:
        raise ValueError(f"B has {B.shape[1]} columns, expected {N}")
    if C is not None and not (C.is_cuda and C.device == B.device and C.is_contiguous() and C.dtype == want
                              and tuple(C.shape) == (info["rows"], N)):
        raise ValueError(f"C must be a contiguous {want} tensor of shape ({info['rows']}, {N}) on {B.device}")
    return want, N


ACTIVATIONS = {None: 0, "relu": 1}  # gs_epilogue.activation (GS_ACT_NONE / GS_ACT_RELU)
_EPILOGUE_KEYS = ("alpha", "bias", "activation", "residual")


def _check_activation(activation):
    """the activation's code; checked before anything touches a device"""
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be None or 'relu', not {activation!r}")
    return ACTIVATIONS[activation]


def _extent(t):
    """[first byte, one past the last byte) of a contiguous tensor or of (pointer, bytes)"""
    if isinstance(t, tuple):
        return t[0], t[0] + t[1]
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def _epilogue(info, device, C, N, alpha=1.0, bias=None, activation=None, residual=None, token_major=False):
    """the gs_epilogue of one SpMM, or None for the identity (alpha 1, nothing else).  Everything is
    checked here, before any launch: the activation's name first, then alpha (finite), bias (a
    contiguous float32 GPU tensor of `rows` elements on `device`) and residual (a contiguous GPU
    tensor of C's dtype and shape on `device` whose memory does not overlap C's).  C: the output
    tensor, (pointer, bytes) for a raw pointer, or None when spmm allocates it.  token_major
    (Plan.linear): C and the residual are (N, rows), the bias still one per row of A."""
    act = _check_activation(activation)
    alpha = float(alpha)
    if not np.isfinite(alpha):
        raise ValueError(f"alpha must be finite, not {alpha}")
    if act == 0 and alpha == 1.0 and bias is None and residual is None:
        return None
    import torch
    want, rows = _torch_dtype(info["dtype"]), info["rows"]
    if bias is not None:
        if not (isinstance(bias, torch.Tensor) and bias.is_cuda and bias.device == device):
            raise ValueError(f"bias must be a GPU tensor on {device}")
        if bias.dtype != torch.float32:
            raise TypeError("bias must be float32")
        if not (bias.dim() == 1 and bias.shape[0] == rows and bias.is_contiguous()):
            raise ValueError(f"bias must be a contiguous vector of {rows} elements (one per row of C)")
    if residual is not None:
        if not (isinstance(residual, torch.Tensor) and residual.is_cuda and residual.device == device):
            raise ValueError(f"residual must be a GPU tensor on {device}")
        if residual.dtype != want:
            raise TypeError(f"residual must be {want}")
        shape = (N, rows) if token_major else (rows, N)
        if not (tuple(residual.shape) == shape and residual.is_contiguous()):
            raise ValueError(f"residual must be a contiguous tensor of shape {shape}")
        if C is not None:
            (r0, r1), (c0, c1) = _extent(residual), _extent(C)
            if r0 < c1 and c0 < r1:
                raise ValueError("residual may not overlap C")
    return _lib.GsEpilogue(alpha, act, bias.data_ptr() if bias is not None else None,
                           residual.data_ptr() if residual is not None else None)


class Batch:
    """a fixed list of SpMMs (plan, replica, B, C) run by gs_spmm_batch: consecutive K-split
    matrix-core entries of one instantiation are one grouped launch (k_mfma_ks_group).  The
    argument arrays are built once; run() enqueues the whole batch on a stream.
    epilogues: per entry None or a dict with any of alpha / bias / activation / residual (as
    Plan.spmm's keywords); the launches are the same with or without them (gs_spmm_batch_ex)."""

    def __init__(self, entries, N, epilogues=None):
        self._L = _lib.load()
        n = len(entries)
        self.plans = [e[0] for e in entries]  # keeps the plans alive
        if epilogues is not None:
            if len(epilogues) != n:
                raise ValueError("epilogues must hold one item (None or a dict) per entry")
            for ep in epilogues:
                if ep is not None:
                    unknown = set(ep) - set(_EPILOGUE_KEYS)
                    if unknown:
                        raise ValueError(f"unknown epilogue keys {sorted(unknown)}")
                    _check_activation(ep.get("activation"))
        for e in entries:
            if not isinstance(e[2], int):
                _check_operands(e[0].info(), e[2], None if isinstance(e[3], int) else e[3], int(N))
        self._epi = None
        if epilogues is not None and any(ep is not None for ep in epilogues):
            self._keep = epilogues  # keeps the bias and residual tensors alive
            self._eps = []
            for e, ep in zip(entries, epilogues):
                if ep is None:
                    self._eps.append(None)
                    continue
                info = e[0].info()
                if isinstance(e[2], int):
                    raise ValueError("an entry with an epilogue needs B as a tensor (its device is checked)")
                ebytes = 4 if info["dtype"] == GS_F32 else 2
                C = (e[3], info["rows"] * int(N) * ebytes) if isinstance(e[3], int) else e[3]
                self._eps.append(_epilogue(info, e[2].device, C, int(N), **ep))
            self._epi = (ctypes.POINTER(_lib.GsEpilogue) * n)(
                *[ctypes.pointer(x) if x is not None else None for x in self._eps])
        self._p = (ctypes.c_void_p * n)(*[e[0]._h for e in entries])
        self._r = (ctypes.c_int * n)(*[int(e[1]) for e in entries])
        self._b = (ctypes.c_void_p * n)(*[e[2] if isinstance(e[2], int) else e[2].data_ptr() for e in entries])
        self._c = (ctypes.c_void_p * n)(*[e[3] if isinstance(e[3], int) else e[3].data_ptr() for e in entries])
        self.n, self.N = n, int(N)

    def run(self, stream=0):
        if self._epi is not None:
            _lib.check(self._L.gs_spmm_batch_ex(self._p, self._r, self._b, self._c, self._epi, self.n, self.N,
                                                ctypes.c_void_p(stream)))
            return
        _lib.check(self._L.gs_spmm_batch(self._p, self._r, self._b, self._c, self.n, self.N, ctypes.c_void_p(stream)))

    def launches(self):
        """entries per launch, as run() enqueues them (gs_batch_launches): a grouped
        k_mfma_ks_group launch carries up to 32 entries"""
        cap = max(1, self.n)
        out = (ctypes.c_int * cap)()
        k = self._L.gs_batch_launches(self._p, self._r, self.n, self.N, out, cap)
        if k < 0:
            _lib.check(k)
        return [out[i] for i in range(min(k, cap))]


def _check_linear_operands(info, x, out):
    """Plan.linear's operands: x a contiguous (n, K) GPU tensor of the plan's dtype, n >= 1; out (or None) a
    contiguous (n, M) tensor of that dtype on x's device.  Returns (dtype, n, M)"""
    want, M, K = _torch_dtype(info["dtype"]), info["rows"], info["cols"]
    if not (x.is_cuda and x.dim() == 2 and x.is_contiguous()):
        raise ValueError("x must be a contiguous 2-D GPU tensor")
    if x.shape[1] != K:
        raise ValueError(f"x has {x.shape[1]} columns, A has {K} columns")
    if x.dtype != want:
        raise TypeError(f"x must be {want}")
    n = int(x.shape[0])
    if n < 1:
        raise ValueError("x holds no token")
    if out is not None and not (out.is_cuda and out.device == x.device and out.is_contiguous() and out.dtype == want
                                and tuple(out.shape) == (n, M)):
        raise ValueError(f"out must be a contiguous {want} tensor of shape ({n}, {M}) on {x.device}")
    return want, n, M


class LinearBatch:
    """a fixed list of linear calls (plan, replica, x, out), each what Plan.linear(x, out, replica) is, run by
    gs_linear_batch: consecutive entries that are each ONE k_mfma_ks_tm launch of one instantiation run as one
    grouped launch (k_mfma_ks_tm_group) -- every entry with its own token count, several may share one x --
    and every other entry through Plan.linear's own path.  An entry's out has the bits of its own
    Plan.linear call.  epilogues: per entry None or a dict with any of alpha / bias / activation / residual
    (Plan.linear's keywords).  The operands are checked and the argument arrays built here, once, before
    anything touches a device; run() enqueues the whole batch on a stream.  Entries that share a plan
    object need distinct replicas to share a launch (Plan.add_replica); launches() tells."""

    def __init__(self, entries, epilogues=None):
        entries = [tuple(e) for e in entries]
        n = len(entries)
        if any(len(e) != 4 for e in entries):
            raise ValueError("an entry is (plan, replica, x, out)")
        if epilogues is not None:
            if len(epilogues) != n:
                raise ValueError("epilogues must hold one item (None or a dict) per entry")
            for ep in epilogues:
                if ep is not None:
                    unknown = set(ep) - set(_EPILOGUE_KEYS)
                    if unknown:
                        raise ValueError(f"unknown epilogue keys {sorted(unknown)}")
                    _check_activation(ep.get("activation"))
        eps, tokens = [], []
        for i, (plan, replica, x, out) in enumerate(entries):
            info = plan.info()
            if not 0 <= int(replica) < max(1, info["replicas"]):
                raise ValueError(f"entry {i}: replica {replica} of a plan with {info['replicas']}")
            if out is None:
                raise ValueError(f"entry {i}: out must be a tensor (the batch allocates nothing)")
            _, tok, _ = _check_linear_operands(info, x, out)
            tokens.append(tok)
            ep = epilogues[i] if epilogues is not None else None
            eps.append(_epilogue(info, x.device, out, tok, token_major=True, **ep) if ep is not None else None)
        self._L = _lib.load()
        self.entries, self._keep, self._eps = entries, epilogues, eps  # keeps plans, operands, bias and residual alive
        self._epi = None
        if any(e is not None for e in eps):
            self._epi = (ctypes.POINTER(_lib.GsEpilogue) * n)(*[ctypes.pointer(e) if e is not None else None for e in eps])
        self._p = (ctypes.c_void_p * n)(*[e[0]._h for e in entries])
        self._r = (ctypes.c_int * n)(*[int(e[1]) for e in entries])
        self._x = (ctypes.c_void_p * n)(*[e[2].data_ptr() for e in entries])
        self._y = (ctypes.c_void_p * n)(*[e[3].data_ptr() for e in entries])
        self._t = (ctypes.c_int * n)(*tokens)
        self.n = n
        self._dev = entries[0][2].device if n else None

    def run(self, stream=None):
        if self.n == 0:
            return
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self._dev).cuda_stream
        _lib.check(self._L.gs_linear_batch(self._p, self._r, self._x, self._y, self._t, self._epi, self.n,
                                           ctypes.c_void_p(stream)))

    def launches(self):
        """entries per launch, as run() enqueues them (gs_linear_batch_launches): a grouped k_mfma_ks_tm_group
        launch carries up to 32 entries; an entry that runs through Plan.linear's path counts as 1"""
        cap = max(1, self.n)
        out = (ctypes.c_int * cap)()
        k = self._L.gs_linear_batch_launches(self._p, self._r, self._x, self._t, self.n, out, cap)
        if k < 0:
            _lib.check(k)
        return [out[i] for i in range(min(k, cap))]


def linear_group_layout(nwg, tiles):
    """begin[] of one grouped token-major launch, host only (gs_linear_group_layout): entry i with nwg[i]
    workgroups per token tile and tiles[i] tiles owns workgroups [begin[i], begin[i] + nwg[i] * tiles[i]); every
    begin is a multiple of 8, begin[-1] is the grid.  Refused: no entry, more than linear_group_max(), an entry
    without workgroups, a grid past 2^31 - 1"""
    n = len(nwg)
    if len(tiles) != n:
        raise ValueError("nwg and tiles must have one length")
    a = (ctypes.c_uint32 * max(1, n))(*[int(v) for v in nwg])
    t = (ctypes.c_uint32 * max(1, n))(*[int(v) for v in tiles])
    out = (ctypes.c_uint32 * (n + 1))()
    _lib.check(_lib.load().gs_linear_group_layout(a, t, n, out))
    return list(out)


def linear_group_max():
    """the most entries of one grouped token-major launch (gs_linear_group_max)"""
    return int(_lib.load().gs_linear_group_max())


class Rotation:
    """`count` SpMMs of one plan from native code (gs_spmm_rotate), rotating its replicas and
    a fixed list of (B, C) pairs: launch i uses pair (first + i) % len(Bs).  The operands are
    checked and the pointer arrays built here, once, so run() adds only the native call."""

    def __init__(self, plan, Bs, Cs):
        n = len(Bs)
        if n == 0 or len(Cs) != n:
            raise ValueError("Bs and Cs must be non-empty lists of one length")
        info = plan.info()
        self.N = int(Bs[0].shape[1])
        for b, c in zip(Bs, Cs):
            _check_operands(info, b, c, self.N)
        self.plan, self.Bs, self.Cs, self.n = plan, Bs, Cs, n  # keeps plan and operands alive
        self._bp = (ctypes.c_void_p * n)(*[b.data_ptr() for b in Bs])
        self._cp = (ctypes.c_void_p * n)(*[c.data_ptr() for c in Cs])
        self._dev = Bs[0].device

    def run(self, count, first=0, stream=None):
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self._dev).cuda_stream
        _lib.check(self.plan._L.gs_spmm_rotate(self.plan._h, int(count), int(first), self._bp, self._cp, self.n,
                                               self.N, ctypes.c_void_p(stream)))


class Plan:
    """A GeneralSparse plan: metadata set + operator history + code generator +
    device copies.  Wraps gs_plan_t."""

    def __init__(self, handle):
        self._h = ctypes.c_void_p(handle)
        self._L = _lib.load()

    # ---------------------------------------------------------------- create
    @classmethod
    def from_mtx(cls, path, ones_values=True):
        """Reference reader semantics by default: every value := 1 (struct.cc:186-200)."""
        L = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(L.gs_plan_create_from_mtx(str(path).encode(), int(bool(ones_values)), ctypes.byref(h)))
        return cls(h.value)

    @classmethod
    def load(cls, path):
        """a compiled plan from a binary plan file (plan_io.cc); upload() before spmm()"""
        L = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(L.gs_plan_load(str(path).encode(), ctypes.byref(h)))
        return cls(h.value)

    def save(self, path):
        """writes the compiled plan (kernel selection + every plan array) to one binary file"""
        _lib.check(self._L.gs_plan_save(self._h, str(path).encode()))
        return self

    @classmethod
    def from_coo(cls, n_rows, n_cols, row, col, val=None):
        """Row-sorted COO; the dims grow to the largest index + 1 (the reference derives them
        from the entries, struct.cc:104-131).  row / col / val must hold the same number of
        entries and the indices must be non-negative integers."""
        L = _lib.load()
        row, col = np.asarray(row), np.asarray(col)
        for name, a in (("row", row), ("col", col)):
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
                raise _refused(f"from_coo: {name} must be a 1-D integer array")
            if a.size and a.min() < 0:
                raise _refused(f"from_coo: negative {name} index")
        if len(col) != len(row) or (val is not None and len(val) != len(row)):
            raise _refused("from_coo: row, col and val lengths differ")
        row = np.ascontiguousarray(row, dtype=np.uint64)
        col = np.ascontiguousarray(col, dtype=np.uint64)
        vp = None
        if val is not None:
            val = np.ascontiguousarray(val, dtype=np.float32)
            vp = val.ctypes.data_as(_lib.f32p)
        h = ctypes.c_void_p()
        _lib.check(L.gs_plan_create_from_coo(int(n_rows), int(n_cols), len(row), row.ctypes.data_as(_lib.u64p),
                                             col.ctypes.data_as(_lib.u64p), vp, ctypes.byref(h)))
        return cls(h.value)

    @classmethod
    def from_scipy(cls, A):
        A = A.tocsr()
        A.sort_indices()
        coo = A.tocoo()
        return cls.from_coo(A.shape[0], A.shape[1], coo.row, coo.col, coo.data)

    # ------------------------------------------------------------ operators
    def add_operator(self, name, *args, sub=0):
        """operator_executer::add_and_run of the named operator on sub-matrix `sub`
        (the reference's code_generator(meta, sub) target)"""
        arr = (ctypes.c_longlong * max(1, len(args)))(*[int(a) for a in args])
        _lib.check(self._L.gs_plan_add_operator_sub(self._h, int(sub), name.encode(), arr, len(args)))
        return self

    def run_pipeline(self, name, N, p0=0, p1=0, sub=0):
        _lib.check(self._L.gs_plan_run_pipeline_sub(self._h, int(sub), name.encode(), int(N), int(p0), int(p1)))
        return self

    def divide_rows(self, interval, sub=0):
        """fixed_interval_row_matrix_div_operator: one new sub-matrix per non-empty interval
        of `interval` rows; returns the live sub-matrix ids"""
        self.add_operator("fixed_interval_row_matrix_div_operator", int(interval), sub=sub)
        return self.sub_matrices()

    def sub_matrices(self):
        n = self._L.gs_plan_sub_matrices(self._h, None, 0)
        _lib.check(min(n, 0))
        ids = (ctypes.c_int * max(1, n))()
        _lib.check(min(self._L.gs_plan_sub_matrices(self._h, ids, n), 0))
        return list(ids[:n])

    def compile(self):
        _lib.check(self._L.gs_plan_compile(self._h))
        return self

    def generate_program(self, root, repeat=100):
        buf = ctypes.create_string_buffer(4096)
        _lib.check(self._L.gs_plan_generate_program(self._h, str(root).encode(), int(repeat), buf, 4096))
        return buf.value.decode()

    # --------------------------------------------------------------- device
    def upload(self, dtype="f16", device=0, *, weights=None, row_scale=None):
        """A's arrays to the device in the layout of the plan's kernel; B and C of every later call hold
        `dtype`.  weights="fp8" (gs_plan_upload_ex, GS_W_FP8_E4M3) stores A's values as OCP e4m3fn codes
        with one float32 scale per row -- row_scale (M values, finite and > 0) or, by default, the power
        of two that brings the row's largest magnitude into (224, 448]: 3 instead of 4 bytes per stored
        entry.  Only for an undivided k_mfma_ks plan built for 17 .. 32 columns, dtype "f16", K a
        multiple of 8; anything else is refused and the plan is then not on the device.  Such a plan runs
        spmm at the width it was built for and linear at any token count; with power-of-two scales the
        results are bit for bit those of an f16 plan of fp8_decode(codes) * scale[row]."""
        self.dtype_code = _dtype_code(dtype)
        self._device = int(device)
        w = _weights_code(weights)
        if w == GS_W_NATIVE:
            if row_scale is not None:
                raise _refused("upload: row_scale goes with weights=\"fp8\"")
            _lib.check(self._L.gs_plan_upload(self._h, self.dtype_code, int(device)))
            return self
        sp = None
        if row_scale is not None:
            row_scale = np.ascontiguousarray(row_scale, dtype=np.float32).ravel()
            rows = self.info()["rows"]
            if row_scale.size != rows:
                raise _refused(f"upload: row_scale must hold one scale per row of A ({rows}), not {row_scale.size}")
            sp = row_scale.ctypes.data_as(_lib.f32p)
        _lib.check(self._L.gs_plan_upload_ex(self._h, self.dtype_code, w, sp, int(device)))
        return self

    def fp8_layout(self, row_scale=None):
        """(codes, scale): the 8-bit value array -- 8 e4m3 codes per entry group of the plan's k_mfma_ks
        layout, pad slots 0 -- and the M scales exactly as upload(weights="fp8", row_scale=row_scale)
        would lay them out under the current config; no device is touched (gs_plan_fp8_layout)"""
        sp = None
        if row_scale is not None:
            row_scale = np.ascontiguousarray(row_scale, dtype=np.float32).ravel()
            if row_scale.size != self.info()["rows"]:
                raise _refused("fp8_layout: row_scale must hold one scale per row of A")
            sp = row_scale.ctypes.data_as(_lib.f32p)
        n = ctypes.c_uint64(0)
        _lib.check(self._L.gs_plan_fp8_layout(self._h, sp, None, 0, ctypes.byref(n), None))
        codes = np.zeros(n.value, np.uint8)
        scale = np.zeros(self.info()["rows"], np.float32)
        _lib.check(self._L.gs_plan_fp8_layout(self._h, sp, codes.ctypes.data_as(_lib.u8p), codes.size, ctypes.byref(n),
                                              scale.ctypes.data_as(_lib.f32p)))
        return codes, scale

    def add_replica(self):
        _lib.check(self._L.gs_plan_add_replica(self._h))

    def spmm(self, B, C=None, replica=0, stream=None, *, alpha=1.0, bias=None, activation=None, residual=None):
        """C = A @ B on the GPU.  B: (K, N) torch tensor on the plan's device, in
        the plan's dtype.  Enqueued on torch's current stream.
        The keywords add an element-wise epilogue (gs_spmm_ex), in this order on the fp32 sums:
        times alpha, plus bias[row] (float32, one per row of C), activation ("relu"), plus residual
        (C's dtype and shape, no overlap with C); C is rounded once.  epilogue_fused(N) tells whether
        the plan applies it inside its kernel or as a pass over C.  Every argument is checked before
        anything is launched, so a refused call leaves C untouched."""
        _check_activation(activation)
        import torch
        info = self.info()
        want, N = _check_operands(info, B, C)
        epi = _epilogue(info, B.device, C, N, alpha, bias, activation, residual)
        if C is None:
            C = torch.empty((info["rows"], N), dtype=want, device=B.device)
        s = stream if stream is not None else torch.cuda.current_stream(B.device).cuda_stream
        if epi is None:
            _lib.check(self._L.gs_spmm_replica(self._h, int(replica), ctypes.c_void_p(B.data_ptr()),
                                               ctypes.c_void_p(C.data_ptr()), int(N), ctypes.c_void_p(s)))
        else:
            _lib.check(self._L.gs_spmm_ex(self._h, int(replica), ctypes.c_void_p(B.data_ptr()),
                                          ctypes.c_void_p(C.data_ptr()), int(N), ctypes.byref(epi), ctypes.c_void_p(s)))
        return C

    def epilogue_fused(self, N):
        """1 when spmm at dense width N applies an epilogue inside its kernel (k_mfma_ks at the
        plan's tile width: one rounding), 0 when it runs as a pass over C after the kernels
        (every other family; 16-bit plans then round twice); gs_plan_epilogue_fused"""
        k = self._L.gs_plan_epilogue_fused(self._h, int(N))
        if k < 0:
            _lib.check(k)
        return k

    def linear(self, x, out=None, replica=0, stream=None, *, alpha=1.0, bias=None, activation=None, residual=None):
        """y = epilogue(x @ A.T) on the GPU, with activations as a linear layer holds them (gs_linear):
        x is a contiguous (n, K) GPU tensor of the plan's dtype, the result (n, M).  out and residual
        are contiguous (n, M) tensors on x's device, residual not overlapping out; bias is float32
        with M entries (one per output feature), so with A the (out, in) weight this is
        F.linear(x, A, bias).  The stages and their order are spmm's.  linear_fused(n) tells whether
        the call is one kernel on x and y in place or three launches through a transposed scratch.
        On a plan that kernel covers (a k_mfma_ks plan built for 17 .. 32 tokens) any n >= 1 runs it,
        on ceil(n / 32) token tiles, and row t of y has the same bits whatever n is and wherever
        token t stands in x; linear_launches(n) tells the launches.
        Every argument is checked before anything is launched, so a refused call leaves out untouched."""
        _check_activation(activation)
        import torch
        info = self.info()
        want, n, M = _check_linear_operands(info, x, out)
        epi = _epilogue(info, x.device, out, n, alpha, bias, activation, residual, token_major=True)
        if out is None:
            out = torch.empty((n, M), dtype=want, device=x.device)
        s = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(self._L.gs_linear(self._h, int(replica), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), n,
                                     ctypes.byref(epi) if epi is not None else None, ctypes.c_void_p(s)))
        return out

    # ------------------------------------------------------------- backward
    def _pattern(self, values=True):
        n = ctypes.c_uint64(0)
        _lib.check(self._L.gs_plan_pattern(self._h, None, None, None, 0, ctypes.byref(n)))
        row, col = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint64)
        val = np.zeros(n.value, np.float32) if values else None
        if n.value:
            _lib.check(self._L.gs_plan_pattern(self._h, row.ctypes.data_as(_lib.u64p), col.ctypes.data_as(_lib.u64p),
                                               val.ctypes.data_as(_lib.f32p) if values else None, n.value, ctypes.byref(n)))
        return row, col, val

    def pattern(self):
        """(row, col) of the plan's entries as uint64 arrays in the canonical order: by original row, then
        by column, stored duplicates adjacent in input order -- np.nonzero's order for a dense weight.
        The same after any pipeline; no device is touched and no value is asked for, so it works while the
        plan's host values are stale (set_values) (gs_plan_pattern)"""
        row, col, _ = self._pattern(values=False)
        return row, col

    def values(self):
        """the float32 values the plan holds on the host, in pattern()'s order; refused (GsError) while they
        are stale: after a set_values that changed the device only"""
        return self._pattern()[2]

    # -------------------------------------------------------- value updates
    def values_prepare(self):
        """builds set_values' map and uploads it now (gs_plan_values_prepare): once per plan, 4 bytes per slot
        of the layout's value array (about the bytes of the plan's A), shared by its replicas; needed before a
        stream capture that holds the plan's first set_values"""
        _lib.check(self._L.gs_plan_values_prepare(self._h))
        return self

    def set_values(self, values, host=False, stream=None):
        """new values for the plan's entries, in pattern()'s order, written into the uploaded plan in place
        (gs_plan_set_values, k_set_values): every replica then holds the bits of a fresh upload of them; the
        plan, its arrays and every Batch / Rotation built on it stay as they are.  Enqueued on torch's current
        stream like a launch; keeping it ordered against launches of this plan on other streams is the caller's job.
        values: a contiguous float32 tensor of nnz elements on the plan's device -- the update then never
        leaves the GPU, and the plan's HOST values become stale: values(), save(), fp8_layout() and the first
        launch at another dense width refuse until a refresh; host=True also copies the tensor to the CPU and
        refreshes them -- or a CPU tensor / numpy array: a host refresh plus the device update through a
        temporary device copy.  Only for k_mfma_ks plans at f16 / bf16 with native weights and no CSR resident
        (GsError otherwise, nothing launched).  Every argument is checked before the call."""
        import torch
        info = self.info()
        nnz = info["nnz"]
        if not info["replicas"]:
            raise _refused("set_values: plan is not on the device")
        dev = torch.device("cuda", getattr(self, "_device", 0))
        if isinstance(values, torch.Tensor) and values.is_cuda:
            if values.device != dev:
                raise ValueError(f"values must be on the plan's device ({dev}), not {values.device}")
            if values.dtype != torch.float32:
                raise TypeError("values must be float32")
            if not (values.dim() == 1 and values.numel() == nnz and values.is_contiguous()):
                raise ValueError(f"values must be a contiguous vector of {nnz} elements (one per entry of pattern())")
            d = values
            h = values.cpu().numpy() if host else None
        else:
            if isinstance(values, torch.Tensor):
                if values.dtype != torch.float32:
                    raise TypeError("values must be float32")
                values = values.detach().numpy()
            h = np.asarray(values)
            if h.dtype != np.float32:
                raise TypeError("values must be float32")
            if not (h.ndim == 1 and h.size == nnz):
                raise ValueError(f"values must be a vector of {nnz} elements (one per entry of pattern())")
            h = np.ascontiguousarray(h)
            d = torch.from_numpy(h if h.flags.writeable else h.copy()).to(dev)  # (torch wants a writable array)
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self._L.gs_plan_set_values(self._h, ctypes.c_void_p(d.data_ptr()),
                                              h.ctypes.data_as(_lib.f32p) if h is not None else None, ctypes.c_void_p(s)))
        if d is not values and stream is not None:
            # (the temporary copy belongs to torch's current stream: it may not be reused before the kernel on
            # the caller's stream has read it)
            torch.cuda.synchronize(dev)
        return self

    def value_sources(self, dtype="f16"):
        """(src, vals16) of the plan's k_mfma_ks layout, host only (gs_plan_value_sources): src[slot] the index
        in pattern()'s order of the entry whose value lives in that slot of the layout's value array
        (0xffffffff: none), vals16 the 16-bit value words exactly as upload(dtype) would lay them out under
        the current config.  GsError for a plan set_values could not update (off k_mfma_ks, a coordinate
        stored twice, ...)."""
        code = _dtype_code(dtype)
        n = ctypes.c_uint64(0)
        _lib.check(self._L.gs_plan_value_sources(self._h, code, None, 0, ctypes.byref(n), None))
        src, vals = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint16)
        _lib.check(self._L.gs_plan_value_sources(self._h, code, src.ctypes.data_as(_lib.u32p), src.size, ctypes.byref(n),
                                                 vals.ctypes.data_as(_lib.u16p)))
        return src, vals

    def sddmm_prepare(self):
        """uploads the pattern for sddmm now (gs_plan_sddmm_prepare): once per plan; needed before a
        stream capture that holds the plan's first sddmm"""
        _lib.check(self._L.gs_plan_sddmm_prepare(self._h))
        return self

    def sddmm(self, g, x, out=None, stream=None):
        """out[e] = sum_t g[t, row_e] * x[t, col_e] over pattern()'s entries (gs_sddmm, k_sddmm_tm): the
        gradient of linear with respect to the weight's stored values.  g: (n, M) and x: (n, K), contiguous
        GPU tensors of the plan's dtype (f16 or bf16; an f32 plan is refused) on the plan's device, n >= 1;
        out: a contiguous float32 tensor of nnz elements there (allocated when None).  fp32 sums in one
        fixed order: the same bits on every call.  Every argument is checked before the call, so a
        refused call leaves out untouched."""
        import torch
        info = self.info()
        M, K, nnz = info["rows"], info["cols"], info["nnz"]
        for name, t, feat in (("g", g, M), ("x", x, K)):
            if not (isinstance(t, torch.Tensor) and t.dim() == 2 and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous 2-D tensor")
            if t.shape[1] != feat:
                raise ValueError(f"{name} has {t.shape[1]} columns, expected {feat}")
            if t.dtype not in (torch.float16, torch.bfloat16):
                raise TypeError(f"{name} must be float16 or bfloat16 (the plan's dtype)")
        n = int(g.shape[0])
        if x.shape[0] != n or n < 1:
            raise ValueError("g and x must hold the same number of tokens, at least one")
        if not info["replicas"]:
            raise _refused("sddmm: plan is not on the device")
        want = _torch_dtype(info["dtype"])
        if g.dtype != want or x.dtype != want:
            raise TypeError(f"g and x must be {want}")
        dev = getattr(self, "_device", None)
        for name, t in (("g", g), ("x", x)):
            if not t.is_cuda or t.device != g.device or (dev is not None and t.device.index != dev):
                raise ValueError(f"{name} must be a GPU tensor on the plan's device")
        if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == g.device
                                    and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == nnz):
            raise ValueError(f"out must be a contiguous float32 tensor of {nnz} elements on {g.device}")
        if out is None:
            out = torch.empty(nnz, dtype=torch.float32, device=g.device)
        s = stream if stream is not None else torch.cuda.current_stream(g.device).cuda_stream
        _lib.check(self._L.gs_sddmm(self._h, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(x.data_ptr()), n,
                                    ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(s)))
        return out

    def linear_fused(self, n):
        """1 when linear at n tokens runs k_mfma_ks_tm (a k_mfma_ks plan built for 17 .. 32 tokens,
        K a multiple of 8, LINEAR_FUSE on; x 16-byte aligned, as torch allocates) -- for such a plan
        at every n >= 1, not only the width it was built for -- 0 when it runs the three-launch
        path; gs_plan_linear_fused"""
        k = self._L.gs_plan_linear_fused(self._h, int(n))
        if k < 0:
            _lib.check(k)
        return k

    def linear_launches(self, n, x=None):
        """the k_mfma_ks_tm launches linear enqueues at n tokens: a list of token tiles (of 32 tokens)
        per launch, in token order -- [ceil(n / 32)] unless the tiles' K-split state would pass
        LINEAR_WS_KB; [] for the three-launch path.  x (optional): the tensor linear would get; one
        that is not 16-byte aligned takes the three launches (without it, alignment is assumed);
        gs_plan_linear_launches"""
        if x is not None and x.data_ptr() % 16:
            self.linear_fused(n)  # (the plan's own errors first)
            return []
        cap = 16
        while True:
            buf = (ctypes.c_int * cap)()
            k = self._L.gs_plan_linear_launches(self._h, int(n), buf, cap)
            if k < 0:
                _lib.check(k)
            if k <= cap:
                return list(buf[:k])
            cap = k

    def rotation(self, Bs, Cs):
        """the (B, C) pairs of spmm_rotate, checked and packed once; .run(count, first) enqueues"""
        return Rotation(self, Bs, Cs)

    def spmm_rotate(self, count, first, Bs, Cs, stream=None):
        """`count` SpMMs from native code, rotating replicas and the (B, C) pairs."""
        self.rotation(Bs, Cs).run(count, first, stream)

    def spmm_raw(self, B_ptr, C_ptr, N, replica=0, stream=0):
        _lib.check(self._L.gs_spmm_replica(self._h, int(replica), ctypes.c_void_p(B_ptr), ctypes.c_void_p(C_ptr),
                                           int(N), ctypes.c_void_p(stream)))

    # ------------------------------------------------------------ inspection
    def info(self):
        i = _lib.GsPlanInfo()
        _lib.check(self._L.gs_plan_info_get(self._h, ctypes.byref(i)))
        return {k: (getattr(i, k).decode() if k in ("kernel_name", "device_kernel") else getattr(i, k))
                for k, _ in i._fields_}

    def keys(self):
        n = self._L.gs_plan_array_count(self._h)
        out = []
        buf = ctypes.create_string_buffer(256)
        for i in range(n):
            _lib.check(self._L.gs_plan_array_key(self._h, i, buf, 256))
            out.append(buf.value.decode())
        return out

    def array(self, key):
        k = key.encode()
        n = self._L.gs_plan_array_len(self._h, k)
        if n < 0:
            raise KeyError(key)
        if self._L.gs_plan_array_is_float(self._h, k) == 1:
            a = np.zeros(n, np.float64)
            _lib.check(self._L.gs_plan_array_read_f64(self._h, k, a.ctypes.data_as(_lib.f64p), n))
        else:
            a = np.zeros(n, np.uint64)
            _lib.check(self._L.gs_plan_array_read_u64(self._h, k, a.ctypes.data_as(_lib.u64p), n))
        return a

    def arrays(self):
        return {k: self.array(k) for k in self.keys()}

    def index_compression(self, key):
        """(kind, expression of i, exact) for one integer plan array (code_generator.cc:2618-3063;
        "none" unless MODEL_DRIVEN_COMPRESS is set)"""
        kind = ctypes.create_string_buffer(32)
        expr = ctypes.create_string_buffer(1 << 14)
        ex = ctypes.c_int(0)
        _lib.check(self._L.gs_plan_index_compression(self._h, key.encode(), kind, 32, expr, 1 << 14, ctypes.byref(ex)))
        return kind.value.decode(), expr.value.decode(), bool(ex.value)

    def logical_check(self):
        """"" when the metadata set is consistent, else the first violation
        (logical_check, metadata_set.cc:806-1890)"""
        buf = ctypes.create_string_buffer(1024)
        rc = self._L.gs_plan_logical_check(self._h, buf, 1024)
        _lib.check(min(rc, 0))
        return buf.value.decode()

    def set_array_entry(self, key, i, value):
        """metadata editing (tools / tests): entry i of an integer plan array"""
        _lib.check(self._L.gs_plan_array_set_u64(self._h, key.encode(), int(i), int(value)))
        return self

    def device_status(self, stream=0):
        """synchronises `stream` and raises GsError (code GS_ERR_DEVICE) if a launch of this
        plan reported a device fault since the last call (gs_plan_device_status: a K-split
        combine that gave up waiting for a partial slab)"""
        _lib.check(self._L.gs_plan_device_status(self._h, ctypes.c_void_p(stream)))
        return self

    def log(self):
        buf = ctypes.create_string_buffer(1 << 16)
        _lib.check(self._L.gs_plan_log(self._h, buf, 1 << 16))
        return buf.value.decode()

    def free(self):
        if self._h is not None and self._h.value:
            self._L.gs_plan_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def __getattr__(name):
    """SparseLinear and SparseLinearGroup live in generalsparse_amd.nn, which needs torch: imported on first use"""
    if name in ("SparseLinear", "SparseLinearGroup"):
        from . import nn
        return getattr(nn, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
