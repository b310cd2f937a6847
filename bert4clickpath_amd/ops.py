"""Host-side operators over libb4c_hip.so: raw launch wrappers plus the block-level
``torch.autograd.Function``s the modules are made of.  PyTorch is used for device
memory, streams and the autograd tape only -- every FLOP and byte below runs in the
hand-written HIP kernels.  No CPU path exists: CPU tensors raise ``B4CError``."""
import ctypes
import os

import torch

from . import _lib as L
from ._lib import B4CError

LN_EPS = 1e-6

_weights_epoch = 0      # bumped by optimizers that write parameters through raw pointers


def bump_weights_epoch():
    global _weights_epoch
    _weights_epoch += 1


def rup8(n):
    return (n + 7) // 8 * 8


# ---- optional launch recorder (bench.py): HIP events on the launch stream around EVERY launch of the hot-path
# kernels, with the algorithmic bytes / flops of that launch, so the dominant kernel family and its roofline
# fraction are measured live inside the timed region -------------------------------------------------------
_rec = None        # None = off; else dict family -> [ms_events..., bytes, flops, launches]
# host-side facts about the batch in flight that the recorder's ALGORITHMIC counts need and the launch sites cannot see
# (the sequence lengths live on the device): bench.py sets them per step.
#   token_rows: rows of the token-sized tensors (T): GEMMs with fewer than half of them are booked as `gemm_nt_rows`
#   sum_len_sq: sum over sequences of len^2 -- the real work of the packed attention (T x S is an upper bound)
#   sum_q_len:  sum over sequences of (masked query rows x len) -- the masked-query attention of the last layer
rec_hints = {}


def set_record_hints(**kw):
    rec_hints.clear()
    rec_hints.update(kw)



def start_recording():
    global _rec
    _rec = {}


def pause_recording():
    """Stop bracketing launches WITHOUT synchronising; hand the result to stop_recording() later."""
    global _rec
    rec, _rec = _rec, None
    return rec


def stop_recording(rec=None):
    """-> {family: {'ms': total, 'launches': n, 'bytes': algorithmic bytes, 'flops': algorithmic flops}} (synchronises)."""
    global _rec
    if rec is None:
        rec, _rec = _rec, None
    torch.cuda.synchronize()
    out = {}
    for fam, items in (rec or {}).items():
        out[fam] = {'ms': sum(a.elapsed_time(b) for a, b, _, _ in items), 'launches': len(items),
                    'bytes': sum(x[2] for x in items), 'flops': sum(x[3] for x in items)}
    return out


# B4C_FAMILY_LOG=<path> (scratch/pmc_traffic.py): EVERY launch that goes through a recorder site is noted, in host order, with
# the family the recorder books it under and its algorithmic bytes -- whether the recorder is on or not.  The PMC script pairs the
# i-th dispatch of a kernel with the i-th note of that kernel's families, so "which launch belongs to which family" has one
# source: this file's `_record(...)` call sites (token-sized and row-sized launches of one kernel are told apart here only).
family_log = [] if os.environ.get('B4C_FAMILY_LOG') else None


def dump_family_log():
    if family_log is not None:
        import json
        with open(os.environ['B4C_FAMILY_LOG'], 'w') as f:
            json.dump(family_log, f)


class _record:
    def __init__(self, family, nbytes, flops=0):
        self.on = _rec is not None
        self.family, self.nbytes, self.flops = family, nbytes, flops
        if family_log is not None:
            family_log.append((family, int(nbytes)))

    def __enter__(self):
        if self.on:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if self.on and _rec is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            _rec.setdefault(self.family, []).append((self.a, b, self.nbytes, self.flops))


_timers = {}


def enable_timer(name):
    _timers[name] = []


def timer_results_ms(name):
    """Mean / count of the recorded launches (call after a device synchronize)."""
    ev = _timers.get(name) or []
    ms = [a.elapsed_time(b) for a, b in ev]
    return (sum(ms) / len(ms) if ms else None), len(ms)


def reset_timer(name):
    if name in _timers:
        _timers[name] = []


class _timed:
    def __init__(self, name):
        self.rec = _timers.get(name)

    def __enter__(self):
        if self.rec is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if self.rec is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            self.rec.append((self.a, b))


def dt_code(dtype):
    if dtype == torch.float32:
        return L.F32
    if dtype == torch.bfloat16:
        return L.BF16
    raise B4CError('unsupported compute dtype %s (float32 or bfloat16)' % dtype)


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise B4CError('bert4clickpath_amd runs on the HIP device only; got a CPU tensor '
                           '(there is no CPU fallback -- move inputs and the model to "cuda")')


# --------------------------------------------------------------------------------------
# raw launches
# --------------------------------------------------------------------------------------
def _feature_arrays(ids_list, tables):
    n = len(ids_list)
    ids_arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ids_list])
    tab_arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tables])
    dims = (ctypes.c_int * n)(*[int(t.shape[1]) for t in tables])
    rows = (ctypes.c_int64 * n)(*[int(t.shape[0]) for t in tables])
    return n, ids_arr, tab_arr, dims, rows


class Packed:
    """Padding-free token layout of one batch (include/b4c.h "packed token layout"): the T real tokens of the (B, S) batch in
    row-major order.  cu [B+1] int32 (sequence b = packed rows cu[b] .. cu[b+1]), tok_src [>= T] int32 (dense position
    b*S + s of packed row t), packed_of [B*S] int32 (inverse, -1 at pads), max_len (upper bound of the longest sequence)."""
    __slots__ = ('cu', 'tok_src', 'packed_of', 'B', 'S', 'T', 'max_len', 'ids_packed')

    def __init__(self, cu, tok_src, packed_of, B, S, T, max_len):
        self.cu, self.tok_src, self.packed_of, self.B, self.S, self.T, self.max_len = cu, tok_src, packed_of, B, S, T, max_len
        self.ids_packed = None


def nonpad_positions(ids, cap, pad_value=0):
    """-> (counts [B], cu [B+1], tok_src [cap], packed_of [B*S], maxcount [1]) (all int32): b4c_nonpad_positions."""
    _cuda(ids)
    B, S = ids.shape
    dev = ids.device
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    cu = torch.empty(B + 1, dtype=torch.int32, device=dev)
    tok_src = zeros(max(cap, 1), dtype=torch.int32, device=dev)      # rows past the true count (wrong cap) read token 0
    packed_of = torch.empty(B * S, dtype=torch.int32, device=dev)
    mx = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(L.lib().b4c_nonpad_positions(_p(ids), B, S, pad_value, _p(counts), _p(cu), _p(tok_src), cap, _p(packed_of), _p(mx),
                                         _st()), 'nonpad_positions')
    return counts, cu, tok_src, packed_of, mx


def remap_index(idx, mapping):
    out = torch.empty_like(idx)
    L.check(L.lib().b4c_remap_index(_p(idx), _p(mapping), _p(out), idx.shape[0], _st()), 'remap_index')
    return out


def _embed_shape(ids_list, tables, pe, combine):
    """-> (B, S, d_model) of an embedding-stage call, after the checks the kernels rely on"""
    _cuda(pe, *ids_list, *tables)
    B, S = ids_list[0].shape
    if combine == 'sum':
        d = int(tables[0].shape[1])
        if len(tables) < 2 or any(int(t.shape[1]) != d for t in tables):
            raise B4CError("combine='sum' needs two or more embedding tables of one width")
    elif combine == 'concat':
        d = sum(int(t.shape[1]) for t in tables)
    else:
        raise B4CError("combine must be 'concat' or 'sum', got %r" % (combine,))
    for i in ids_list:
        if i.dtype != torch.int64 or not i.is_contiguous() or tuple(i.shape) != (B, S):
            raise B4CError('embedding ids must be contiguous int64 (B,S) tensors of one shape')
    for t in tables:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise B4CError('embedding tables must be contiguous float32')
    if pe.shape[0] < S or pe.shape[1] != d:
        raise B4CError('positional table (%d,%d) too small for S=%d d=%d' % (pe.shape[0], pe.shape[1], S, d))
    return B, S, d


def embed_concat_pe_fwd(ids_list, tables, pe, scale, rate, seed, dtype, packed=None, combine='concat'):
    """combine='sum' (two or more features of one width): the gathered rows are added instead of concatenated -- the
    library takes that form when every table is d_model wide."""
    B, S, d = _embed_shape(ids_list, tables, pe, combine)
    n, ids_arr, tab_arr, dims, rows = _feature_arrays(ids_list, tables)
    if packed is not None:      # rows of the real tokens only
        T_tok = packed.T
        out = torch.empty(1, T_tok, d, dtype=dtype, device=pe.device)
        key_pad = torch.empty(T_tok, dtype=torch.uint8, device=pe.device)
        with _record('embed_fwd', T_tok * d * (4 + out.element_size())):
            L.check(L.lib().b4c_embed_concat_pe_fwd_packed(n, ids_arr, tab_arr, dims, rows, _p(pe), scale, _p(out), d, _p(key_pad),
                                                           B, S, d, rate, seed, _p(packed.tok_src), T_tok, dt_code(dtype), _st()),
                    'embed_concat_pe_fwd_packed')
        return out, key_pad
    out = torch.empty(B, S, d, dtype=dtype, device=pe.device)
    key_pad = torch.empty(B, S, dtype=torch.uint8, device=pe.device)
    with _record('embed_fwd', B * S * d * (4 + out.element_size())):
        L.check(L.lib().b4c_embed_concat_pe_fwd(n, ids_arr, tab_arr, dims, rows, _p(pe), scale, _p(out), d, _p(key_pad),
                                                B, S, d, rate, seed, dt_code(dtype), _st()), 'embed_concat_pe_fwd')
    return out, key_pad


library_sort = True      # b4c_sort_ids (2 launches per 8-bit pass) instead of torch.sort (14 launches through rocPRIM)


# ---- scratch memory the library's entry points take from the caller -----------------------------------------------------
# One growing buffer per (purpose, device, launch stream): launches of ONE stream use it one after the other, so the stream
# order keeps them apart; two models that train on streams of their own get buffers of their own (a buffer shared across
# streams would be written by two kernels at once).  Nothing here belongs to a training step: the buffers hold no results.
_workspaces = {}


def _workspace(kind, device, need, floor=0):
    """uint8 scratch tensor of at least `need` bytes for launches of `kind` on `device`'s current stream"""
    key = (kind, device, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(int(need), int(floor), 1), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


_dense_cu = {}


def dense_cu(B, S, device):
    """int32 [B + 1] = b * S: the first row of every sequence of the dense (B, S) layout (built once per shape and device)"""
    key = (B, S, device)
    if key not in _dense_cu:
        _dense_cu[key] = torch.arange(B + 1, dtype=torch.int32, device=device) * S
    return _dense_cu[key]


def pos_table_bwd(dout, cu, B, S, rate, seed, into, row_of=None):
    """into [>= S, d] (fp32) += the embedding stage's gradient w.r.t. a learned positional table (b4c_pos_table_bwd):
    dout [T, d] the stage's output gradient, cu [B+1] int32 first row of every sequence (b * S in the dense layout), or
    row_of [B*S] int32 (Packed.packed_of: the row of every dense position, -1 = none) for the packed layout;
    rate / seed: the forward's dropout.  Fixed summation order: the same bits on every launch."""
    d = dout.shape[-1]
    dout = dout.reshape(-1, d)
    if into.dtype != torch.float32 or not into.is_contiguous() or into.shape[0] < S or into.shape[1] != d:
        raise B4CError('pos_table_bwd: the gradient table must be contiguous float32 [>= %d, %d]' % (S, d))
    if row_of is not None:
        if row_of.dtype != torch.int32 or row_of.numel() != B * S or not row_of.is_contiguous():
            raise B4CError('pos_table_bwd: row_of must be a contiguous int32 [B * S] tensor')
    elif cu is None or cu.dtype != torch.int32 or cu.numel() != B + 1 or not cu.is_contiguous():
        raise B4CError('pos_table_bwd: cu must be a contiguous int32 [B + 1] tensor')
    ws = _workspace('pos_table_bwd', dout.device, L.lib().b4c_pos_table_bwd_workspace_bytes(B, S, d))
    with _record('pos_table_bwd', dout.shape[0] * d * dout.element_size() + S * d * 4):
        L.check(L.lib().b4c_pos_table_bwd(_p(dout), dout.stride(0), dout.shape[0], _p(cu), _p(row_of), B, S, d, rate, seed, _p(into),
                                          ws.data_ptr(), ws.numel(), dt_code(dout.dtype), _st()), 'pos_table_bwd')
    return into


def _sort_order(ids, n_rows):
    """Token indices sorted by id (int32).  Radix-sort cost grows with the key width, and ids are row indices of a
    table: 16-bit keys for tables of up to 65,536 rows (biased into int16), else 32-bit (63 / 178 / 224 us for 16 / 32 / 64
    bits at 819,200 tokens).  Out-of-range ids are clamped exactly as the kernels clamp them."""
    if library_sort and ids.is_cuda:
        flat = ids.reshape(-1)
        if flat.dtype != torch.int64 or not flat.is_contiguous():
            flat = flat.to(torch.int64).contiguous()
        n = flat.shape[0]
        order = torch.empty(n, dtype=torch.int32, device=ids.device)
        if n == 0:
            return order
        need = L.lib().b4c_sort_ids_workspace_bytes(n, n_rows)
        ws = _workspace('sort', ids.device, need, 1 << 20)
        L.check(L.lib().b4c_sort_ids(_p(flat), n, n_rows, _p(order), ws.data_ptr(), ws.numel(), _st()), 'sort_ids')
        return order
    flat = ids.view(-1).clamp(0, n_rows - 1)
    if n_rows <= 65536:
        keys = (flat - 32768).to(torch.int16)
    else:
        keys = flat.to(torch.int32)
    return torch.sort(keys, stable=True)[1].to(torch.int32)


sorted_embed_bwd = True     # sort the tokens of every feature by id (one radix sort per call) and sum runs in registers

# ops.deterministic (on by default; B4C_DETERMINISTIC=0 switches it off): ONE switch for a bit-reproducible training step --
# every reduction that otherwise finishes through float atomics (whose arrival order, and with it the last bit of the sum,
# changes from run to run, and training carries such differences on into every later step) takes a fixed-order form instead:
#   the vocabulary projection's dW / db      the token splits of the sweep store partial sums in the workspace, added in split
#                                            order (background pieces: one workgroup per vocabulary tile walks every token);
#                                            label term through a stable sort
#   the embedding tables' gradient rows      runs of one id that cross the kernel's 64-entry ranges are summed in range order
#                                            (b4c_embed_concat_pe_bwd_sorted_ws); the unsorted atomic kernel is never taken
#   LayerNorm dgamma / dbeta                 per-workgroup sums in a fixed order, added block by block (b4c_add_dropout_layernorm_bwd_ws)
# (the dense weight gradients already are: ops.tn_deterministic).  Not covered: the sampled-softmax head's row scatter (config 5).
# Two identical runs of bench.py's step then give torch.equal arenas (tests/test_gpu_deterministic.py); cost: DESIGN.md.
deterministic = os.environ.get('B4C_DETERMINISTIC', '1') == '1'


def embed_concat_pe_bwd(ids_list, tables, dout, scale, rate, seed, into=None, order=None):
    B, S = ids_list[0].shape
    d = dout.shape[-1]
    dtabs = into if into is not None else [torch.zeros_like(t) for t in tables]
    n, ids_arr, tab_arr, dims, rows = _feature_arrays(ids_list, dtabs)
    if (sorted_embed_bwd and B * S >= 4096) or deterministic:
        if order is None:
            order = [_sort_order(i, int(t.shape[0])) for i, t in zip(ids_list, tables)]
        ord_arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in order])
        ws = None
        if deterministic:
            ws = _workspace('embed_bwd', dout.device, L.lib().b4c_embed_concat_pe_bwd_sorted_workspace_bytes(n, dims, B, S))
        with _record('embed_bwd', B * S * d * (4 + dout.element_size())):
            L.check(L.lib().b4c_embed_concat_pe_bwd_sorted_ws(n, ids_arr, ord_arr, tab_arr, dims, rows, scale, _p(dout), d, B, S, d,
                                                              rate, seed, _p(ws), ws.numel() if ws is not None else 0,
                                                              dt_code(dout.dtype), _st()), 'embed_concat_pe_bwd_sorted')
        return dtabs
    with _record('embed_bwd', B * S * d * (4 + dout.element_size())):
        L.check(L.lib().b4c_embed_concat_pe_bwd(n, ids_arr, tab_arr, dims, rows, scale, _p(dout), d, B, S, d, rate, seed,
                                                dt_code(dout.dtype), _st()), 'embed_concat_pe_bwd')
    return dtabs


def _embed_ln_shape(ids_list, tables, pe, combine):
    """_embed_shape for the LayerNorm form, whose kernels also read pe in the backward: contiguous float32"""
    if pe.dtype != torch.float32 or not pe.is_contiguous():
        raise B4CError('embed_ln: the positional table must be contiguous float32')
    return _embed_shape(ids_list, tables, pe, combine)


def _ln_vectors(d, *vs):
    for v in vs:
        if v.dtype != torch.float32 or not v.is_contiguous() or tuple(v.shape) != (d,):
            raise B4CError('LayerNorm gamma / beta / their gradient sinks must be contiguous float32 [%d]' % d)


def _rows_view(t, T_tok, d, dtype, what):
    """a caller-given [T, d] output (any leading shape, unit column stride, 16-B rows) as the kernels take it"""
    t2 = t.reshape(-1, t.shape[-1]) if t.is_contiguous() else t
    if t2.dtype != dtype or tuple(t2.shape) != (T_tok, d) or t2.stride(1) != 1 or (t2.stride(0) * t2.element_size()) % 16 or \
            t2.data_ptr() % 16:
        raise B4CError('%s must be a [%d, %d] %s tensor with unit column stride and 16-B aligned rows' % (what, T_tok, d, dtype))
    return t2


def embed_ln_fwd(ids_list, tables, pe, scale, gamma, beta, rate, seed, dtype, packed=None, combine='concat', eps=LN_EPS,
                 out=None, stats=None):
    """The embedding stage with LayerNorm (b4c_embed_ln_fwd): drop(LayerNorm(scale * rows + pe)) -> (out, key_pad, stats);
    out (B, S, d), or (1, T, d) with `packed`; stats fp32 [T, 2] = (mean, rstd) of every row.  out / stats: tensors to write
    into (a [T, d] view with unit column stride; a contiguous [T, 2])."""
    B, S, d = _embed_ln_shape(ids_list, tables, pe, combine)
    _cuda(gamma, beta)
    _ln_vectors(d, gamma, beta)
    n, ids_arr, tab_arr, dims, rows = _feature_arrays(ids_list, tables)
    T_tok = packed.T if packed is not None else B * S
    dev = pe.device
    if out is None:
        out = torch.empty((1, T_tok, d) if packed is not None else (B, S, d), dtype=dtype, device=dev)
    o2 = _rows_view(out, T_tok, d, dtype, 'embed_ln_fwd: out')
    if stats is None:
        stats = torch.empty(T_tok, 2, dtype=torch.float32, device=dev)
    elif stats.dtype != torch.float32 or not stats.is_contiguous() or tuple(stats.shape) != (T_tok, 2):
        raise B4CError('embed_ln_fwd: stats must be a contiguous float32 [%d, 2] tensor' % T_tok)
    key_pad = torch.empty((T_tok,) if packed is not None else (B, S), dtype=torch.uint8, device=dev)
    with _record('embed_ln_fwd', T_tok * d * (4 + o2.element_size()) + 8 * T_tok):
        L.check(L.lib().b4c_embed_ln_fwd(n, ids_arr, tab_arr, dims, rows, _p(pe), scale, _p(gamma), _p(beta), eps, _p(o2),
                                         o2.stride(0), _p(stats), _p(key_pad), B, S, d, rate, seed,
                                         _p(packed.tok_src) if packed is not None else None, T_tok, dt_code(dtype), _st()),
                'embed_ln_fwd')
    return out, key_pad, stats


def embed_ln_bwd(ids_list, tables, pe, scale, gamma, stats, dout, rate, seed, packed=None, combine='concat', into=None,
                 dpre=None, workspace=None):
    """Backward of embed_ln_fwd up to the pre-norm row (b4c_embed_ln_bwd) -> (dpre, dgamma, dbeta).  ids_list: the DENSE (B, S)
    ids of the forward call (with `packed`, rows are taken through packed.tok_src as there); dout [T, d] in the compute dtype.
    into = (dgamma, dbeta): fp32 [d] sinks that are added to.  The tables' and a learned pe's gradients follow from dpre through
    embed_concat_pe_bwd / pos_table_bwd at rate 0.  Fixed summation order: the same bits on every launch."""
    B, S, d = _embed_ln_shape(ids_list, tables, pe, combine)
    T_tok = packed.T if packed is not None else B * S
    g2 = _rows_view(dout, T_tok, d, dout.dtype, 'embed_ln_bwd: dout')
    dt_code(g2.dtype)
    _cuda(gamma, stats, g2)
    if into is not None:
        dgamma, dbeta = into
    else:
        dgamma, dbeta = zeros(d, device=g2.device), zeros(d, device=g2.device)
    _ln_vectors(d, gamma, dgamma, dbeta)
    if stats.dtype != torch.float32 or not stats.is_contiguous() or tuple(stats.shape) != (T_tok, 2):
        raise B4CError('embed_ln_bwd: stats must be the contiguous float32 [%d, 2] tensor of the forward call' % T_tok)
    if dpre is None:
        dpre = torch.empty(T_tok, d, dtype=g2.dtype, device=g2.device)
    p2 = _rows_view(dpre, T_tok, d, g2.dtype, 'embed_ln_bwd: dpre')
    if T_tok == 0:
        return dpre, dgamma, dbeta
    n, ids_arr, tab_arr, dims, rows = _feature_arrays(ids_list, tables)
    ws = workspace if workspace is not None else _workspace('ln_bwd', g2.device, L.lib().b4c_embed_ln_bwd_workspace_bytes(T_tok, d))
    with _record('embed_ln_bwd', T_tok * d * (4 + 2 * g2.element_size()) + 8 * T_tok):
        L.check(L.lib().b4c_embed_ln_bwd(n, ids_arr, tab_arr, dims, rows, _p(pe), scale, _p(gamma), _p(stats), _p(g2), g2.stride(0),
                                         _p(p2), p2.stride(0), _p(dgamma), _p(dbeta), B, S, d, rate, seed,
                                         _p(packed.tok_src) if packed is not None else None, T_tok, ws.data_ptr(),
                                         ws.numel() * ws.element_size(), dt_code(g2.dtype), _st()), 'embed_ln_bwd')
    return dpre, dgamma, dbeta


def row_pitch(n):
    """Row pitch (elements) of a materialised [rows, n] vocabulary-wide tensor: n rounded up to 128 elements, so that every
    row starts on a 256-B boundary.  With V = 50,000 a bf16 row is 100,000 B and starts 32 B further into a 128-B line
    than the row above it: a pure store kernel with the projection's tile shape then writes 3.8 TB/s, with aligned rows
    5.5 TB/s (scratch/store_bw2.hip).  Narrow outputs keep their natural pitch."""
    return n if n < 2048 else (n + 127) // 128 * 128


def empty_rows(R, n, dtype, device):
    """An uninitialised [R, n] tensor on the row_pitch(n) pitch (a view of a [R, pitch] allocation; contiguous when the
    pitch is n)."""
    ld = row_pitch(n)
    buf = torch.empty(R, ld, dtype=dtype, device=device)
    return buf if ld == n else buf[:, :n]


def zero_(t):
    """zeros into a contiguous tensor through the library (hipMemsetAsync on the launch stream), in place"""
    if t.is_cuda and t.is_contiguous():
        if t.numel():
            L.check(L.lib().b4c_zero(_p(t), t.numel() * t.element_size(), _st()), 'zero')
        return t
    return t.zero_()


def zeros(*shape, dtype=torch.float32, device=None):
    """torch.zeros through the library's fill on a GPU (no PyTorch kernel in the training step's trace)"""
    t = torch.empty(*shape, dtype=dtype, device=device)
    return zero_(t) if t.is_cuda else t.zero_()


def chain_ids(seqs, cls, sep):
    """[cls, sep, seq_0, sep, seq_1, sep, ...] along axis 1 for (B, L_i) int64 id tensors on a GPU (b4c_chain_ids)"""
    B = seqs[0].shape[0]
    seqs = [s if (s.stride(-1) == 1 or s.shape[1] == 0) else s.contiguous() for s in seqs]
    S = 2 + sum(int(s.shape[1]) + 1 for s in seqs)
    out = torch.empty(B, S, dtype=torch.int64, device=seqs[0].device)
    n = len(seqs)
    ptrs = (ctypes.c_void_p * n)(*[s.data_ptr() for s in seqs])
    lens = (ctypes.c_int * n)(*[int(s.shape[1]) for s in seqs])
    pitches = (ctypes.c_int * n)(*[int(s.stride(0)) if s.shape[1] else 0 for s in seqs])
    L.check(L.lib().b4c_chain_ids(ptrs, lens, pitches, n, B, int(cls), int(sep), _p(out), S, _st()), 'chain_ids')
    return out


def _rows_ok(g, dtype):
    """g as the kernels take it: `dtype`, unit column stride, 16-B aligned rows -- copied only when it is not"""
    if g.dtype != dtype:
        g = g.to(dtype)
    if g.dim() != 2 or g.stride(1) != 1 or (g.stride(0) * g.element_size()) % 16 or g.data_ptr() % 16:
        g = g.contiguous()
    return g


FFN_ACTIVATIONS = {'relu': L.ACT_RELU, 'gelu': L.ACT_GELU, 'gelu_tanh': L.ACT_GELU_TANH}


def ffn_act_code(name):
    """B4C_ACT_* of a feed-forward activation name ('relu' | 'gelu' | 'gelu_tanh'); anything else is a ValueError"""
    try:
        return FFN_ACTIVATIONS[name]
    except (KeyError, TypeError):
        raise ValueError("ffn_activation must be 'relu', 'gelu' or 'gelu_tanh', got %r" % (name,)) from None


def gemm_nt(a, bt, n, bias=None, act=L.ACT_NONE, gate=None, residual=None, out_dtype=None, out=None, gate_act=L.ACT_RELU,
            pre=None):
    """a: [M, Kp], bt: [>=n, Kp] -> [M, n] (written into `out`, a row-pitched [M, n] view, when given).
    gate_act: how `gate` is applied (ACT_RELU: the gate's sign; a GELU: act'(gate), gate = the saved pre-activation).
    pre: an [M, n] tensor of a's dtype that also receives the pre-activation acc + bias (b4c_gemm_nt_act)."""
    M, K = a.shape
    out_dtype = out_dtype or a.dtype
    if out is None:
        out = torch.empty(M, n, dtype=out_dtype, device=a.device)
    elif out.dtype != out_dtype or tuple(out.shape) != (M, n) or out.stride(1) != 1:
        raise B4CError('gemm_nt: out must be a [%d, %d] %s view with unit column stride' % (M, n, out_dtype))
    if M == 0:
        return out
    es = a.element_size()
    nbytes = M * K * es + n * K * es + M * n * out.element_size() + (M * n * es if gate is not None else 0) + \
        (M * n * es if residual is not None else 0) + (M * n * es if pre is not None else 0)
    if pre is not None and (pre.dtype != a.dtype or tuple(pre.shape) != (M, n) or pre.stride(1) != 1):
        raise B4CError('gemm_nt: pre must be a [%d, %d] %s view with unit column stride' % (M, n, a.dtype))
    # the materialised vocabulary projection (wide kernel: bf16, K <= 128, N >= 2048, plain epilogue) is its own family
    fam = 'vocab_proj' if (n >= 2048 and K <= 128 and a.dtype == torch.bfloat16 and out_dtype == torch.bfloat16 and
                           act == L.ACT_NONE and gate is None and residual is None) else 'gemm_nt'
    # token-sized launches ([T] rows: HBM-bound at 60 - 130 us each) and row-sized ones ([R] rows of the head trunk -- 10 - 60 us
    # each, matrix work -- and of the rows-only last layer, a few us each) are two families: one number would describe neither
    if fam == 'gemm_nt' and 2 * M < rec_hints.get('token_rows', 0):
        fam = 'gemm_nt_rows'
    if pre is not None or gate_act != L.ACT_RELU or act in (L.ACT_GELU, L.ACT_GELU_TANH):
        with _record(fam, nbytes, 2 * M * n * K):
            L.check(L.lib().b4c_gemm_nt_act(_p(a), a.stride(0), _p(bt), bt.stride(0), _p(out), out.stride(0), M, n, K, _p(bias), act,
                                            _p(gate), gate.stride(0) if gate is not None else 0, gate_act,
                                            _p(residual), residual.stride(0) if residual is not None else 0,
                                            _p(pre), pre.stride(0) if pre is not None else 0,
                                            dt_code(a.dtype), dt_code(out_dtype), _st()), 'gemm_nt_act')
        return out
    with _record(fam, nbytes, 2 * M * n * K):
        L.check(L.lib().b4c_gemm_nt(_p(a), a.stride(0), _p(bt), bt.stride(0), _p(out), out.stride(0), M, n, K, _p(bias), act,
                                    _p(gate), gate.stride(0) if gate is not None else 0,
                                    _p(residual), residual.stride(0) if residual is not None else 0,
                                    dt_code(a.dtype), dt_code(out_dtype), _st()), 'gemm_nt')
    return out


def gemm_tn(a, g, K, N, want_bias=True, into=None):
    """dW[K,N] (+)= a[:, :K]^T @ g[:, :N] (fp32), db[N] (+)= colsum(g).
    into = (list of dW_i [K, N/len], list of db_i [N/len]): accumulate into existing fp32 tensors (column
    segments of equal width) instead of allocating zeros; returns (None, None) then."""
    M = a.shape[0]
    if M > 0 and (_rec is not None or family_log is not None):
        with _record('gemm_tn' if 2 * M >= rec_hints.get('token_rows', 0) else 'gemm_tn_rows',
                     M * (K + N) * a.element_size() + K * N * 4, 2 * M * K * N):
            return _gemm_tn_impl(a, g, K, N, want_bias, into)
    return _gemm_tn_impl(a, g, K, N, want_bias, into)


tn_deterministic = True     # False: no workspace, partial tiles are added with float atomics


def _tn_workspace(a, M, K, N):
    if not tn_deterministic or M == 0:
        return None, 0
    need = L.lib().b4c_gemm_tn_workspace_bytes(M, K, N, dt_code(a.dtype))
    if need == 0:
        return None, 0
    ws = _workspace('gemm_tn', a.device, need, 32 << 20)      # the split partial tiles of gemm_tn
    return ws.data_ptr(), ws.numel()


def _gemm_tn_impl(a, g, K, N, want_bias, into):
    M = a.shape[0]
    wsp, wsb = _tn_workspace(a, M, K, N)
    if into is not None:
        dWs, dbs = into
        if M == 0:
            return None, None
        n = len(dWs)
        if n == 1:
            L.check(L.lib().b4c_gemm_tn(_p(a), a.stride(0), _p(g), g.stride(0), _p(dWs[0]), N, _p(dbs[0]), M, K, N,
                                        dt_code(a.dtype), wsp, wsb, _st()), 'gemm_tn')
        else:
            wa = (ctypes.c_void_p * n)(*[t.data_ptr() for t in dWs])
            ba = (ctypes.c_void_p * n)(*[t.data_ptr() for t in dbs])
            L.check(L.lib().b4c_gemm_tn_seg(_p(a), a.stride(0), _p(g), g.stride(0), n, wa, ba, N // n, M, K,
                                            dt_code(a.dtype), wsp, wsb, _st()), 'gemm_tn_seg')
        return None, None
    dW = torch.zeros(K, N, dtype=torch.float32, device=a.device)
    db = torch.zeros(N, dtype=torch.float32, device=a.device) if want_bias else None
    if M == 0:
        return dW, db
    L.check(L.lib().b4c_gemm_tn(_p(a), a.stride(0), _p(g), g.stride(0), _p(dW), N, _p(db), M, K, N,
                                dt_code(a.dtype), wsp, wsb, _st()), 'gemm_tn')
    return dW, db


# ---- the whole backward of a Dense layer in one pass over its gradient (csrc/gemm_dxdw.hip) -----------------------------------
# Inside the C2 step (456 k token rows; main kernel + the fixed-order reduction of the workgroups' partial sums):
#   Q | K | V projection (three column blocks)   ~150 us against 111 + 147 us for b4c_gemm_nt + its share of the grouped b4c_gemm_tn
#   K | V of the masked-query last layer (two)    ~100 us against 84 + 91
#   attention output projection (one, no residual) ~70 us against 50 + 50
# B4C_FUSED_DXDW: 0 = off, 1 = Q | K | V only, 2 = + K | V, 3 (default) = + the output projection.
fused_dxdw = int(os.environ.get('B4C_FUSED_DXDW', '3'))


def dxdw_supported(x, g, n_seg, residual=None):
    """bf16, 128-wide layer input, gradient of 128 x n_seg columns (n_seg 1 to 3), rows the kernels' 16-B accesses can take; a
    residual's chunks are addressed with 32-bit byte offsets (b4c_gemm_dxdw refuses M * pitch * 2 >= 2^32)"""
    return x.dtype == torch.bfloat16 and g.dtype == torch.bfloat16 and x.shape[1] == 128 and n_seg in (1, 2, 3) and \
        g.shape[1] == 128 * n_seg and x.stride(0) % 8 == 0 and g.stride(0) % 8 == 0 and x.shape[0] >= 4096 and \
        (residual is None or x.shape[0] * residual.stride(0) * 2 < (1 << 32))


def gemm_dxdw(x, g, wc, dWs, dbs, residual=None):
    """dX = g wc^T (+ residual), dW_s += x^T g_s, db_s += colsum(g_s) with g read once (b4c_gemm_dxdw).
    x [M, 128], g [M, 128 n_seg], wc [128, >= 128 n_seg] (the dX operand of gemm_nt), dWs / dbs: fp32 gradient tensors."""
    M, n_seg = x.shape[0], len(dWs)
    dx = torch.empty(M, 128, dtype=x.dtype, device=x.device)
    ws = _workspace('gemm_dxdw', x.device, L.lib().b4c_gemm_dxdw_workspace_bytes(M, n_seg))
    wa = (ctypes.c_void_p * n_seg)(*[t.data_ptr() for t in dWs])
    ba = (ctypes.c_void_p * n_seg)(*[(t.data_ptr() if t is not None else None) for t in dbs])
    es = 2
    with _record('gemm_dxdw', M * (128 * (1 + n_seg) + 128 + (128 if residual is not None else 0)) * es, 4 * M * 128 * 128 * n_seg):
        L.check(L.lib().b4c_gemm_dxdw(_p(x), x.stride(0), _p(g), g.stride(0), _p(wc), wc.stride(0), _p(residual),
                                      residual.stride(0) if residual is not None else 0, _p(dx), dx.stride(0), n_seg, wa, ba,
                                      dWs[0].stride(0), M, ws.data_ptr(), ws.numel(), _st()), 'gemm_dxdw')
    return dx


# ---- the feed-forward block's whole backward in one pass (csrc/ffn_bwd.hip): LayerNorm + dropout backward, both Dense layers' dX,
# dW and db.  B4C_FUSED_FFN_BWD=0 keeps the five kernels.
fused_ffn_bwd = os.environ.get('B4C_FUSED_FFN_BWD', '1') != '0'


def ffn_bwd_shape_ok(x, h, z):
    """the model shapes b4c_ffn_bwd takes: bf16, d_model = 128, dff <= 128 (padded to 8)"""
    return x.dtype == torch.bfloat16 and h.dtype == torch.bfloat16 and z.dtype == torch.bfloat16 and x.shape[1] == 128 and \
        h.shape[1] <= 128 and h.shape[1] % 8 == 0 and x.stride(0) % 8 == 0 and h.stride(0) % 8 == 0 and z.is_contiguous()


def ffn_bwd_supported(x, h, z):
    """... and enough rows for a persistent kernel (below 4,096 the five kernels are launched), fewer than 2^24 (b4c_ffn_bwd addresses
    its row chunks with 32-bit byte offsets)"""
    return ffn_bwd_shape_ok(x, h, z) and 4096 <= x.shape[0] < (1 << 24)


def ffn_bwd(dout, z, stats, gamma, rate, seed, h, x, wc2, wc1, F, dW1, db1, dW2, db2, dgamma, dbeta):
    """dX of the feed-forward block; dW1 / db1 / dW2 / db2 / dgamma / dbeta += (b4c_ffn_bwd).  wc2 [Fp][>= 128], wc1 [128][>= Fp]:
    the dX operands of gemm_nt for the second / first Dense layer."""
    M, Fp = x.shape[0], h.shape[1]
    dx = torch.empty(M, 128, dtype=x.dtype, device=x.device)
    ws = _workspace('ffn_bwd', x.device, L.lib().b4c_ffn_bwd_workspace_bytes(M))
    es = 2
    with _record('ffn_bwd' if 2 * M >= rec_hints.get('token_rows', 0) else 'ffn_bwd_rows', M * ((4 * 128 + Fp) * es + 8),
                 8 * M * 128 * Fp):
        L.check(L.lib().b4c_ffn_bwd(_p(dout), _p(z), _p(stats), _p(gamma), rate, seed, _p(h), h.stride(0), _p(x), x.stride(0),
                                    _p(wc2), wc2.stride(0), _p(wc1), wc1.stride(0), F, Fp, _p(dx), dx.stride(0),
                                    _p(dW1), dW1.stride(0), _p(db1), _p(dW2), dW2.stride(0), _p(db2), _p(dgamma), _p(dbeta),
                                    M, ws.data_ptr(), ws.numel(), _st()), 'ffn_bwd')
    return dx


# ---- the feed-forward block's forward in one pass (csrc/ffn_fwd.hip).  B4C_FUSED_FFN_FWD=0 keeps gemm_nt + gemm_nt_add_ln.
fused_ffn_fwd = os.environ.get('B4C_FUSED_FFN_FWD', '1') != '0'


def ffn_fwd_supported(x, Fp):
    return x.dtype == torch.bfloat16 and x.shape[1] == 128 and Fp <= 128 and Fp % 8 == 0 and x.stride(0) % 8 == 0 and x.shape[0] >= 4096


def ffn_fwd(x, wt1, b1, wt2, b2, gamma, beta, F, Fp, rate, seed, save=True):
    """-> h [M, Fp], z (None unless save), out, stats (None unless save) of LayerNorm(x + dropout(relu(x W1 + b1) W2 + b2)) (b4c_ffn_fwd).
    wt1 [Fp][128], wt2 [128][Fp]: the forward operands of gemm_nt for the two layers; b1 [Fp], b2 [128] fp32."""
    M = x.shape[0]
    h = torch.empty(M, Fp, dtype=x.dtype, device=x.device)
    z = torch.empty(M, 128, dtype=x.dtype, device=x.device) if save else None
    out = torch.empty(M, 128, dtype=x.dtype, device=x.device)
    stats = torch.empty(M, 2, dtype=torch.float32, device=x.device) if save else None
    with _record('ffn_fwd' if 2 * M >= rec_hints.get('token_rows', 0) else 'ffn_fwd_rows',
                 M * ((128 * (3 if save else 2) + Fp) * 2 + (8 if save else 0)), 4 * M * 128 * Fp):
        L.check(L.lib().b4c_ffn_fwd(_p(x), x.stride(0), _p(wt1), wt1.stride(0), _p(b1), _p(wt2), wt2.stride(0), _p(b2), _p(gamma), _p(beta),
                                    F, Fp, _p(h), h.stride(0), _p(z), _p(out), _p(stats), M, LN_EPS, rate, seed, _st()), 'ffn_fwd')
    return h, z, out, stats


# ---- the fused feed-forward kernels for a GELU block (csrc/ffn_act_fwd.hip, ffn_act_bwd.hip).  Off by default: B4C_FUSED_FFN_GELU=1
# sends a GELU block of the fused shape through them (where fused_ffn_fwd / fused_ffn_bwd allow the ReLU kernels); off, a GELU
# block keeps gemm_nt_act + gemm_nt_add_ln forward and the five kernels backward.
fused_ffn_gelu = os.environ.get('B4C_FUSED_FFN_GELU', '0') == '1'


def ffn_act_fwd(x, wt1, b1, wt2, b2, gamma, beta, F, Fp, act, rate, seed, save=True):
    """-> h [M, Fp], u (None unless save), z (None unless save), out, stats (None unless save) of
    LayerNorm(x + dropout(act(x W1 + b1) W2 + b2)), act a GELU (b4c_ffn_act_fwd); u = x W1 + b1, h = act(u).  Operands as ffn_fwd."""
    M = x.shape[0]
    h = torch.empty(M, Fp, dtype=x.dtype, device=x.device)
    u = torch.empty(M, Fp, dtype=x.dtype, device=x.device) if save else None
    z = torch.empty(M, 128, dtype=x.dtype, device=x.device) if save else None
    out = torch.empty(M, 128, dtype=x.dtype, device=x.device)
    stats = torch.empty(M, 2, dtype=torch.float32, device=x.device) if save else None
    with _record('ffn_act_fwd' if 2 * M >= rec_hints.get('token_rows', 0) else 'ffn_act_fwd_rows',
                 M * ((128 * (3 if save else 2) + Fp * (2 if save else 1)) * 2 + (8 if save else 0)), 4 * M * 128 * Fp):
        L.check(L.lib().b4c_ffn_act_fwd(_p(x), x.stride(0), _p(wt1), wt1.stride(0), _p(b1), _p(wt2), wt2.stride(0), _p(b2), _p(gamma),
                                        _p(beta), F, Fp, act, _p(h), h.stride(0), _p(u), u.stride(0) if save else 0, _p(z), _p(out),
                                        _p(stats), M, LN_EPS, rate, seed, _st()), 'ffn_act_fwd')
    return h, u, z, out, stats


def ffn_act_bwd(dout, z, stats, gamma, rate, seed, act, h, u, x, wc2, wc1, F, dW1, db1, dW2, db2, dgamma, dbeta):
    """dX of a GELU feed-forward block; dW1 / db1 / dW2 / db2 / dgamma / dbeta += (b4c_ffn_act_bwd).  u: the saved pre-activation;
    the other operands as ffn_bwd."""
    M, Fp = x.shape[0], h.shape[1]
    dx = torch.empty(M, 128, dtype=x.dtype, device=x.device)
    ws = _workspace('ffn_bwd', x.device, L.lib().b4c_ffn_bwd_workspace_bytes(M))
    es = 2
    with _record('ffn_act_bwd' if 2 * M >= rec_hints.get('token_rows', 0) else 'ffn_act_bwd_rows', M * ((4 * 128 + 2 * Fp) * es + 8),
                 8 * M * 128 * Fp):
        L.check(L.lib().b4c_ffn_act_bwd(_p(dout), _p(z), _p(stats), _p(gamma), rate, seed, act, _p(h), h.stride(0), _p(u), u.stride(0),
                                        _p(x), x.stride(0), _p(wc2), wc2.stride(0), _p(wc1), wc1.stride(0), F, Fp, _p(dx), dx.stride(0),
                                        _p(dW1), dW1.stride(0), _p(db1), _p(dW2), dW2.stride(0), _p(db2), _p(dgamma), _p(dbeta),
                                        M, ws.data_ptr(), ws.numel(), _st()), 'ffn_act_bwd')
    return dx


# ---- the attention block's tail in one pass (csrc/attn_out_bwd.hip): LayerNorm + dropout backward and the output projection's dX /
# dW / db.  B4C_FUSED_ATTN_OUT_BWD=0 keeps add_ln_bwd + the projection's own kernels.
fused_attn_out_bwd = os.environ.get('B4C_FUSED_ATTN_OUT_BWD', '1') != '0'


def attn_out_bwd_supported(o, z):
    return o.dtype == torch.bfloat16 and z.dtype == torch.bfloat16 and o.shape[1] == 128 and z.shape[1] == 128 and \
        o.stride(0) % 8 == 0 and z.is_contiguous() and 4096 <= o.shape[0] < (1 << 24)     # (32-bit byte offsets of the row chunks)


def attn_out_bwd(dout, z, stats, gamma, rate, seed, o, wc, dW, db, dgamma, dbeta):
    """-> dz [M, 128] (residual branch), d_o [M, 128];  dW / db / dgamma / dbeta += (b4c_attn_out_bwd).  wc [128][>= 128]: the dX
    operand of gemm_nt for the output projection."""
    M = o.shape[0]
    dz = torch.empty(M, 128, dtype=o.dtype, device=o.device)
    d_o = torch.empty(M, 128, dtype=o.dtype, device=o.device)
    ws = _workspace('attn_out_bwd', o.device, L.lib().b4c_attn_out_bwd_workspace_bytes(M))
    with _record('attn_out_bwd' if 2 * M >= rec_hints.get('token_rows', 0) else 'attn_out_bwd_rows', M * (5 * 128 * 2 + 8), 4 * M * 128 * 128):
        L.check(L.lib().b4c_attn_out_bwd(_p(dout), _p(z), _p(stats), _p(gamma), rate, seed, _p(o), o.stride(0), _p(wc), wc.stride(0),
                                         _p(dz), _p(d_o), d_o.stride(0), _p(dW), dW.stride(0), _p(db), _p(dgamma), _p(dbeta),
                                         M, ws.data_ptr(), ws.numel(), _st()), 'attn_out_bwd')
    return dz, d_o


# ---- grouped weight gradients: the dW GEMMs of an encoder layer are off the critical path (nothing in backward
# consumes them), so in arena mode they are queued and launched together (b4c_gemm_tn_group: one main + one reduce
# kernel per layer instead of four of each, and ~6x less partial-tile traffic).
grouped_dw = True


def queue_dw(c, a, g, K, N, dWs, dbs, params):
    """dW_i += a^T g (column segments), db_i += colsum(g) -- now or with the next flush_pending_dw(c).  `c`: the ArenaContext
    of the step in flight (the queue lives there: a step that fails leaves nothing behind for the next one)."""
    ok = _arena_routes(c) and grouped_dw and a.dtype == torch.bfloat16 and a.stride(0) % 8 == 0 and g.stride(0) % 8 == 0 and \
        a.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0 and a.shape[0] >= 4096
    if not ok:
        gemm_tn(a, g, K, N, into=(dWs, dbs))
        _ready(*params)
        return
    q = c.pending_dw
    if q and (q[0][0].shape[0] != a.shape[0] or len(q) == 8):
        flush_pending_dw(c)
    q.append((a, g, K, N, dWs, dbs, params))


def flush_pending_dw(c):
    if c is None or not c.pending_dw:
        return
    items = list(c.pending_dw)
    del c.pending_dw[:]
    M = items[0][0].shape[0]
    descs = (L.TNDesc * len(items))()
    nbytes = flops = 0
    for d, (a, g, K, N, dWs, dbs, _) in zip(descs, items):
        d.A, d.G, d.lda, d.ldg, d.K = a.data_ptr(), g.data_ptr(), a.stride(0), g.stride(0), K
        d.n_seg, d.seg_width, d.ldw = len(dWs), N // len(dWs), dWs[0].stride(0)
        for i, (w, b) in enumerate(zip(dWs, dbs)):
            d.dW[i] = w.data_ptr()
            d.db[i] = b.data_ptr() if b is not None else None
        nbytes += M * (K + N) * a.element_size() + K * N * 4
        flops += 2 * M * K * N
    need = L.lib().b4c_gemm_tn_group_workspace_bytes(descs, len(items), M)
    ws = _workspace('gemm_tn', items[0][0].device, need, 32 << 20)
    with _record('gemm_tn' if 2 * M >= rec_hints.get('token_rows', 0) else 'gemm_tn_rows', nbytes, flops):
        L.check(L.lib().b4c_gemm_tn_group(descs, len(items), M, L.BF16, ws.data_ptr(), ws.numel(), _st()), 'gemm_tn_group')
    for it in items:
        _ready(*it[6])


# ---- per-arena host state ------------------------------------------------------------------------------------------
# optim.FlatArena re-homes parameters and their gradients into two flat buffers.  Every autograd block adds its weight
# gradients into sinks (grad_sinks): in an arena param.grad itself (autograd receives None for those inputs), without one
# fresh zeros that autograd receives (sink_returns).  Everything the host keeps about such a training
# step -- who is told when a gradient is complete, and the side-stream work of the backward pass in flight -- lives in
# the arena's ArenaContext, reachable from every parameter of the arena as `p._b4c_ctx`.  Nothing here is process
# state: two models, with or without an arena, train side by side in one process (tests/test_gpu_context.py).
flash_ce = True          # bf16 training: vocabulary projection + CE without the (R x V) logits (csrc/vocab_ce.hip)


class ArenaContext:
    def __init__(self):
        self.grad_ready_cb = None     # parallel.GradReducer: called with each parameter whose gradient has just been produced
        # weight-gradient GEMMs of the layer in flight, queued for one grouped launch (queue_dw / flush_pending_dw): the
        # entries hold that step's activations and gradient tensors
        self.pending_dw = []
        # side-stream work (the vocabulary head's background dW sweep, see "Vocabulary-head weight gradient BESIDE ...")
        self.queue = []               # closures to run on the side stream, in order: pieces of sweeps, label terms, event records
        self.pending = []             # (event recorded on the side stream, parameters whose gradient it completes, main stream)
        self.slots = 0                # launch opportunities left in the current plan (one now, one per attention backward expected)
        self.counting = False         # inside a backward pass that feeds the queue
        self.kicks = 0                # attention-backward launches seen in this pass
        self.kicks_expected = 0       # ... in the previous backward pass: the plan of the next one
        self.side_launched = None     # device whose side stream has been given work since the last join (None: nothing in flight)
        # the model's feed-forward blocks take the fused backward (FFNBlockFn.forward sets it; the head's backward then runs its dW
        # sweep in the foreground: _background_dw_for)
        self.fused_blocks = False

    def reset(self):
        """Drop what a failed step left behind: queued weight-gradient GEMMs and side-stream closures hold that step's tensors
        and would add a stale gradient into the next one; side-stream kernels that step ALREADY launched (the first piece of the
        background sweep goes out before anything can fail) add into the gradient arena with float atomics, so the stream that
        is about to zero the arena waits for them first.  Called at the start of every step: FlatArena.zero_grad,
        GradReducer.begin_backward."""
        del self.pending_dw[:]
        del self.queue[:]
        if self.side_launched is not None:
            torch.cuda.current_stream(self.side_launched).wait_stream(_side_stream(self.side_launched))
            self.side_launched = None
        del self.pending[:]
        self.slots = self.kicks = 0
        self.counting = False


def arena_context(*params):
    """The ArenaContext shared by all of `params` whose .grad is a live view of that arena's gradient buffer, else None."""
    ctx = None
    for p in params:
        c = getattr(p, '_b4c_ctx', None)
        g = p.grad
        if c is None or (ctx is not None and c is not ctx):
            return None
        if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
            return None
        ctx = c
    return ctx


def grad_sinks(*params):
    """-> (actx, sinks): where the backward kernels add each parameter's fp32 gradient.  In an arena (actx = arena_context(...))
    sinks[i] is params[i].grad, the arena's view; otherwise a fresh zero tensor of the parameter's shape, handed to autograd by
    sink_returns."""
    actx = arena_context(*params)
    if actx is not None:
        return actx, [p.grad for p in params]
    return None, [torch.zeros(p.shape, dtype=torch.float32, device=p.device) for p in params]


def sink_returns(ctx, lead, actx, sinks):
    """autograd's return values of a block: `lead` for the inputs in front of its parameters, then per parameter its sink (None in
    an arena: the kernels have already added into .grad), then None for every input after them"""
    out = tuple(lead) + ((None,) * len(sinks) if actx is not None else tuple(sinks))
    return out + (None,) * (len(ctx.needs_input_grad) - len(out))


def _arena_routes(actx):
    # the fused backward kernels, the grouped dW queue and the background sweep run in arena mode only, as they always have
    return actx is not None


def _ready(*params):
    for p in params:
        c = getattr(p, '_b4c_ctx', None)
        if c is not None and c.grad_ready_cb is not None:
            c.grad_ready_cb(p)


def _tied_table_steps_whole(table):
    """called where a tied projection (TiedPackedLinear) adds its dW into rows off .. off + V of its table, read in this step
    or not: under a row-lazy optimizer (optim.LazyRows) the whole table then takes the next step, as the dense update would
    (the gather sites' row notes cover the rows the embedding read, not these)"""
    lz = getattr(table, '_b4c_lazy', None)
    if lz is not None:
        lz.all_rows = True


def _attn_mq_drop(q_rows, rate, causal=False):
    rate = _attn_rate(rate)
    if rate > 0 and q_rows is None:
        raise ValueError('attention dropout in the masked-query kernels needs q_rows (the token row of each query row)')
    if causal and q_rows is None:
        raise ValueError('causal attention in the masked-query kernels needs q_rows (the token row of each query row)')
    return rate


def _attn_mq_pairs(R, max_len, causal):
    """(query, key) pairs of a masked-query launch for the work hint: rec_hints['sum_q_len'] (every query row against its sequence),
    for a causal launch rec_hints['sum_q_visible'] (the sum of p + 1 over the query rows) when the caller gives it; R x max_len
    is the upper bound of both"""
    if causal and 'sum_q_visible' in rec_hints:
        return rec_hints['sum_q_visible']
    return rec_hints.get('sum_q_len', R * max_len)


def attn_mq_fwd(q, kv, cu, moff, B, max_len, H, dh, key_pad=None, q_rows=None, rate=0.0, seed=0, causal=False):
    """Attention of a few query rows per sequence against all of its keys (b4c_attn_mq_fwd_drop; rate 0 launches the kernels of
    b4c_attn_mq_fwd).
    q [R, H*dh]; kv [T, 2*H*dh] (k | v); cu [B+1] token offsets; moff [B+1] query-row offsets -> (o [R, H*dh], lse [R, H]).
    rate > 0: dropout on the attention probabilities with the masks attn_fwd(..., rate, seed) draws for the
    token rows q_rows [R] (int32; an unused row holds -1): b4c_attn_keep(seed, b, h, q_rows[r] - cu[b], k, H, max_len, rate).
    causal (b4c_attn_mq_fwd_ex with B4C_ATTN_CAUSAL; needs q_rows): query row r sees the keys 0 .. q_rows[r] - cu[b] of its
    sequence, the rows attn_fwd(..., causal=True) computes at those positions; a row inside a range whose q_rows is below cu[b]
    (-1) sees none: o = 0, lse = 0.  Without it the calls are the ones made before there was such a form."""
    rate = _attn_mq_drop(q_rows, rate, causal)
    R = q.shape[0]
    # rows outside every [moff[b], moff[b+1]) range (the unused tail of the sync-free form) are not written: zeros, not garbage
    o = zeros(R, H * dh, dtype=q.dtype, device=q.device)
    lse = zeros(R, H, dtype=torch.float32, device=q.device)
    if R == 0:
        return o, lse
    es = q.element_size()
    # algorithmic work: every query row against the keys of its own sequence (host hint; R x max_len is an upper bound)
    with _record('attn_mq_fwd', kv.shape[0] * 2 * H * dh * es + 2 * R * H * dh * es, 4 * _attn_mq_pairs(R, max_len, causal) * H * dh):
        if causal:
            L.check(L.lib().b4c_attn_mq_fwd_ex(_p(q), q.stride(0), _p(kv), kv.stride(0), _p(key_pad), _p(cu), _p(moff), _p(o), o.stride(0),
                                               _p(lse), B, max_len, H, dh, dt_code(q.dtype), _st(), _p(q_rows), rate, seed, L.ATTN_CAUSAL),
                    'attn_mq_fwd_ex')
        else:
            L.check(L.lib().b4c_attn_mq_fwd_drop(_p(q), q.stride(0), _p(kv), kv.stride(0), _p(key_pad), _p(cu), _p(moff), _p(o), o.stride(0),
                                                 _p(lse), B, max_len, H, dh, dt_code(q.dtype), _st(), _p(q_rows), rate, seed), 'attn_mq_fwd_drop')
    return o, lse


def attn_mq_bwd(q, kv, cu, moff, o, d_o, lse, B, max_len, H, dh, key_pad=None, q_rows=None, rate=0.0, seed=0, causal=False):
    """-> (dq [R, H*dh], dkv [T, 2*H*dh]); every token row of dkv is written (zeros where no query reads the sequence; causal:
    also behind a sequence's last query position).
    q_rows, rate, seed, causal: those of the forward (attn_mq_fwd); o is the forward's output, dropped probabilities included."""
    rate = _attn_mq_drop(q_rows, rate, causal)
    R = q.shape[0]
    dq = zeros(q.shape[0], q.shape[1], dtype=q.dtype, device=q.device)
    if R == 0:                 # no query row anywhere: no key or value receives a gradient from this layer
        return dq, torch.zeros_like(kv)
    dkv = torch.empty_like(kv)
    if kv.shape[0] == 0:
        return dq, dkv
    es = q.element_size()
    with _record('attn_mq_bwd', kv.shape[0] * 4 * H * dh * es + 4 * R * H * dh * es, 10 * _attn_mq_pairs(R, max_len, causal) * H * dh):
        if causal:
            L.check(L.lib().b4c_attn_mq_bwd_ex(_p(q), q.stride(0), _p(kv), kv.stride(0), _p(key_pad), _p(cu), _p(moff), _p(o), o.stride(0),
                                               _p(d_o), d_o.stride(0), _p(lse), _p(dq), dq.stride(0), _p(dkv), dkv.stride(0), B, max_len, H, dh,
                                               dt_code(q.dtype), _st(), _p(q_rows), rate, seed, L.ATTN_CAUSAL), 'attn_mq_bwd_ex')
        else:
            L.check(L.lib().b4c_attn_mq_bwd_drop(_p(q), q.stride(0), _p(kv), kv.stride(0), _p(key_pad), _p(cu), _p(moff), _p(o), o.stride(0),
                                                 _p(d_o), d_o.stride(0), _p(lse), _p(dq), dq.stride(0), _p(dkv), dkv.stride(0), B, max_len, H, dh,
                                                 dt_code(q.dtype), _st(), _p(q_rows), rate, seed), 'attn_mq_bwd_drop')
    return dq, dkv


def _attn_rate(rate):
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError('attention dropout rate must lie in [0, 1), got %r' % (rate,))
    return rate


ATTN_CAUSAL = L.ATTN_CAUSAL        # B4C_ATTN_CAUSAL of include/b4c.h (flags of the b4c_attn_*_ex entry points)


def _attn_pairs(T_tok, S, cu, causal):
    """(query, key) pairs a launch works on, for the roofline table.  Bidirectional: sum of len^2 (packed layout: the host hint
    'sum_len_sq'; T x S is an upper bound and what the padded layout computes).  Causal: the triangle, sum of len (len + 1) / 2 --
    skipped tiles are not credited; sum len is the token count, so the same hint serves."""
    pairs = rec_hints.get('sum_len_sq', T_tok * S) if cu is not None else T_tok * S
    return (pairs + T_tok) // 2 if causal else pairs


def attn_fwd(qkv, key_pad, B, S, H, dh, cu=None, rate=0.0, seed=0, causal=False):
    """cu (int32 [B+1]): packed layout -- sequence b owns rows cu[b] .. cu[b+1] of qkv, S = upper bound of the longest one.
    rate > 0: dropout on the attention probabilities, mask b4c_attn_keep(seed, b, h, q, k, H, S, rate) (include/b4c.h); lse is that
    of the undropped softmax.  rate == 0 launches the kernels without dropout.
    causal: key k is visible to query q iff k <= q (B4C_ATTN_CAUSAL); lse is over the visible keys.
    Always b4c_attn_fwd_ex: the layout, the rate and the flags select the launch, and cu = None, rate = 0, flags = 0 is the
    launch of b4c_attn_fwd."""
    rate = _attn_rate(rate)
    if long_attn and S > 512 and attn_long_supported(qkv.dtype, S, dh):
        return attn_long_fwd(qkv, key_pad, B, S, H, dh, cu=cu, rate=rate, seed=seed, causal=causal)
    d = H * dh
    T_tok = qkv.shape[0]
    o = torch.empty(T_tok, d, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=qkv.device)
    with _record('attn_fwd', T_tok * 4 * d * qkv.element_size(), 4 * _attn_pairs(T_tok, S, cu, causal) * d):
        L.check(L.lib().b4c_attn_fwd_ex(_p(qkv), qkv.stride(0), _p(key_pad), _p(cu), _p(o), d, _p(lse), B, S, H, dh,
                                        dt_code(qkv.dtype), _st(), rate, seed, ATTN_CAUSAL if causal else 0), 'attn_fwd_ex')
    return o, lse


def attn_bwd(qkv, key_pad, o, d_o, lse, B, S, H, dh, cu=None, actx=None, rate=0.0, seed=0, causal=False):
    """actx: the ArenaContext of the training step in flight (its background work gets a launch opportunity behind this kernel)
    rate, seed, causal: those of the forward (attn_fwd); o is the forward's output, dropped probabilities included."""
    rate = _attn_rate(rate)
    if long_attn and S > 512 and attn_long_supported(qkv.dtype, S, dh):
        return attn_long_bwd(qkv, key_pad, o, d_o, lse, B, S, H, dh, cu=cu, actx=actx, rate=rate, seed=seed, causal=causal)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    need = L.lib().b4c_attn_bwd_workspace_bytes(B, S, H, dh, dt_code(qkv.dtype))     # > 0 only for bf16 256 < S <= 512
    ws = _workspace('attn_bwd', qkv.device, need) if need else None
    T_tok = qkv.shape[0]
    with _record('attn_bwd', T_tok * 8 * H * dh * qkv.element_size(), 10 * _attn_pairs(T_tok, S, cu, causal) * H * dh):
        L.check(L.lib().b4c_attn_bwd_ex(_p(qkv), qkv.stride(0), _p(key_pad), _p(cu), _p(o), o.stride(0), _p(d_o), d_o.stride(0),
                                        _p(lse), _p(delta), _p(dqkv), dqkv.stride(0), B, S, H, dh, _p(ws), need,
                                        dt_code(qkv.dtype), _st(), rate, seed, ATTN_CAUSAL if causal else 0), 'attn_bwd_ex')
    _background_kick(actx)      # the next piece of the vocabulary head's dW sweep starts when this kernel has left the CUs
    return dqkv


# Sequences past the resident bf16 MFMA kernels (512 < S <= 2048): the streamed kernels of include/b4c.h instead of the
# fp32-math row kernels (dense layout) or a refusal (packed layout).  Off (B4C_ATTN_LONG=1 switches it on): with it off every launch,
# message and result is what it was without these kernels.
long_attn = os.environ.get('B4C_ATTN_LONG', '0') == '1'
ATTN_LONG_MAX_S = L.ATTN_LONG_MAX_S


def attn_long_supported(dtype, S, dh):
    """what b4c_attn_long_fwd / _bwd take: bf16, head depth 32 / 64, 1 <= S <= 2048 (the routing of attn_fwd / attn_bwd adds
    S > 512 and the switch long_attn)"""
    return dtype == torch.bfloat16 and dh in (32, 64) and 1 <= S <= ATTN_LONG_MAX_S


def attn_long_fwd(qkv, key_pad, B, S, H, dh, cu=None, rate=0.0, seed=0, causal=False):
    """attn_fwd on the streamed kernels (b4c_attn_long_fwd): same arguments, layouts, dropout masks and results (o, lse)"""
    rate = _attn_rate(rate)
    d = H * dh
    T_tok = qkv.shape[0]
    o = torch.empty(T_tok, d, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=qkv.device)
    with _record('attn_fwd', T_tok * 4 * d * qkv.element_size(), 4 * _attn_pairs(T_tok, S, cu, causal) * d):
        L.check(L.lib().b4c_attn_long_fwd(_p(qkv), qkv.stride(0), _p(key_pad), _p(cu), _p(o), d, _p(lse), B, S, H, dh, _st(), rate, seed,
                                          ATTN_CAUSAL if causal else 0), 'attn_long_fwd')
    return o, lse


def attn_long_bwd(qkv, key_pad, o, d_o, lse, B, S, H, dh, cu=None, actx=None, rate=0.0, seed=0, causal=False):
    """attn_bwd on the key-block walk (b4c_attn_long_bwd); the fp32 dQ accumulator [rows, H dh] comes from _workspace"""
    rate = _attn_rate(rate)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    T_tok = qkv.shape[0]
    need = L.lib().b4c_attn_long_bwd_workspace_bytes(T_tok, H, dh)
    if need < 0:
        raise B4CError('attn_long_bwd: head depth %d not in {32, 64}' % dh)
    ws = _workspace('attn_long_bwd', qkv.device, need)
    with _record('attn_bwd', T_tok * 8 * H * dh * qkv.element_size(), 10 * _attn_pairs(T_tok, S, cu, causal) * H * dh):
        L.check(L.lib().b4c_attn_long_bwd(_p(qkv), qkv.stride(0), _p(key_pad), _p(cu), _p(o), o.stride(0), _p(d_o), d_o.stride(0),
                                          _p(lse), _p(delta), _p(dqkv), dqkv.stride(0), B, S, H, dh, _p(ws), ws.numel(), _st(), rate, seed,
                                          ATTN_CAUSAL if causal else 0), 'attn_long_bwd')
    _background_kick(actx)
    return dqkv


def add_dropout_layernorm_fwd(x, y, gamma, beta, rate, seed, save=True):
    rows, d = x.shape
    z = torch.empty_like(x) if save else None
    out = torch.empty_like(x)
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device) if save else None
    if rows == 0:
        return z, out, stats
    with _record('add_ln_fwd', rows * d * x.element_size() * (4 if save else 3)):
        L.check(L.lib().b4c_add_dropout_layernorm_fwd(_p(x), _p(y), _p(gamma), _p(beta), _p(z), _p(out), _p(stats), rows, d,
                                                      LN_EPS, rate, seed, dt_code(x.dtype), _st()), 'add_dropout_layernorm_fwd')
    return z, out, stats


fused_ln = True      # bf16, d_model <= 256: the GEMM in front of "x + dropout(y) -> LayerNorm" does it in its epilogue


def gemm_ln_supported(a, n):
    return fused_ln and a.dtype == torch.bfloat16 and n <= 256 and n % 8 == 0


def gemm_nt_add_ln(a, bt, bias, x, gamma, beta, rate, seed, save=True):
    """LayerNorm(x + dropout(a @ bt^T + bias)) in one kernel (== gemm_nt + add_dropout_layernorm_fwd, bit for bit).
    a: [M, Kp], bt: [>=n, Kp], x: [M, n] -> (z, out, stats) as add_dropout_layernorm_fwd."""
    M, K = a.shape
    n = x.shape[1]
    z = torch.empty_like(x) if save else None
    out = torch.empty_like(x)
    stats = torch.empty(M, 2, dtype=torch.float32, device=x.device) if save else None
    if M == 0:
        return z, out, stats
    es = a.element_size()
    with _record('gemm_nt_ln' if 2 * M >= rec_hints.get('token_rows', 0) else 'gemm_nt_ln_rows',
                 M * K * es + n * K * es + M * n * es * (3 if save else 2), 2 * M * n * K):
        L.check(L.lib().b4c_gemm_nt_add_ln(_p(a), a.stride(0), _p(bt), bt.stride(0), _p(bias), _p(x), x.stride(0), _p(gamma),
                                           _p(beta), _p(z), _p(out), _p(stats), M, n, K, LN_EPS, rate, seed,
                                           dt_code(a.dtype), _st()), 'gemm_nt_add_ln')
    return z, out, stats


def add_dropout_layernorm_bwd(dout, z, stats, gamma, rate, seed, into=None):
    rows, d = z.shape
    dz = torch.empty_like(z)
    dy = torch.empty_like(z) if rate > 0 else None
    if into is not None:
        dgamma, dbeta = into
    else:
        dgamma = torch.zeros(d, dtype=torch.float32, device=z.device)
        dbeta = torch.zeros(d, dtype=torch.float32, device=z.device)
    if rows == 0:          # no row at all (a batch without a [MASK]): nothing to add to dgamma / dbeta
        return dz, (dy if dy is not None else dz), dgamma, dbeta
    ws = _workspace('ln_bwd', z.device, L.lib().b4c_add_dropout_layernorm_bwd_workspace_bytes(rows, d)) if deterministic else None
    with _record('add_ln_bwd' if 2 * rows >= rec_hints.get('token_rows', 0) else 'add_ln_bwd_rows',
                 rows * d * z.element_size() * (4 if rate > 0 else 3)):
        L.check(L.lib().b4c_add_dropout_layernorm_bwd_ws(_p(dout), _p(z), _p(stats), _p(gamma), _p(dz), _p(dy), _p(dgamma),
                                                         _p(dbeta), rows, d, rate, seed, _p(ws), ws.numel() if ws is not None else 0,
                                                         dt_code(z.dtype), _st()),
                'add_dropout_layernorm_bwd')
    return dz, (dy if dy is not None else dz), dgamma, dbeta


def layernorm_fwd(x, gamma, beta, eps=LN_EPS, out=None, stats=None):
    """Plain LayerNorm over the rows of x [rows, d] (b4c_layernorm_fwd) -> (out, stats fp32 [rows, 2] = mean, rstd)"""
    rows, d = x.shape
    _cuda(x, gamma, beta)
    _ln_vectors(d, gamma, beta)
    if not x.is_contiguous():
        raise B4CError('layernorm_fwd: x must be contiguous')
    out = torch.empty_like(x) if out is None else out
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device) if stats is None else stats
    if out.dtype != x.dtype or out.shape != x.shape or not out.is_contiguous() or stats.dtype != torch.float32 or \
            tuple(stats.shape) != (rows, 2) or not stats.is_contiguous():
        raise B4CError('layernorm_fwd: out must be contiguous like x, stats a contiguous float32 [%d, 2]' % rows)
    if rows == 0:
        return out, stats
    with _record('layernorm_fwd', rows * d * x.element_size() * 2 + 8 * rows):
        L.check(L.lib().b4c_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(out), _p(stats), rows, d, eps, dt_code(x.dtype), _st()),
                'layernorm_fwd')
    return out, stats


def layernorm_bwd(dout, x, stats, gamma, into=None, gate=None, gate_act=L.ACT_RELU, dx=None, workspace=None):
    """Backward of layernorm_fwd (b4c_layernorm_bwd) -> (dx, dgamma, dbeta); into = (dgamma, dbeta): fp32 [d] sinks, added to.
    gate [rows, d]: dx is multiplied by act'(gate) as it is stored (gate_act: ACT_RELU = the gate's sign, a GELU = its derivative
    at the saved pre-activation) -- the activation in front of the norm.  Fixed summation order: the same bits every launch."""
    rows, d = x.shape
    _cuda(dout, x, stats, gamma)
    if into is not None:
        dgamma, dbeta = into
    else:
        dgamma, dbeta = zeros(d, device=x.device), zeros(d, device=x.device)
    _ln_vectors(d, gamma, dgamma, dbeta)
    dx = torch.empty_like(x) if dx is None else dx
    if dout.dtype != x.dtype or dout.shape != x.shape or not dout.is_contiguous() or not x.is_contiguous() or \
            dx.dtype != x.dtype or dx.shape != x.shape or not dx.is_contiguous():
        raise B4CError('layernorm_bwd: dout, x and dx must be contiguous tensors of one shape and dtype')
    if stats.dtype != torch.float32 or tuple(stats.shape) != (rows, 2) or not stats.is_contiguous():
        raise B4CError('layernorm_bwd: stats must be the contiguous float32 [%d, 2] tensor of the forward call' % rows)
    if gate is not None and (gate.dtype != x.dtype or tuple(gate.shape) != (rows, d) or gate.stride(1) != 1 or
                             (gate.stride(0) * gate.element_size()) % 16 or gate.data_ptr() % 16):
        raise B4CError('layernorm_bwd: gate must be a [%d, %d] %s view with unit column stride' % (rows, d, x.dtype))
    if rows == 0:
        return dx, dgamma, dbeta
    ws = workspace if workspace is not None else _workspace('ln_bwd', x.device, L.lib().b4c_layernorm_bwd_workspace_bytes(rows, d))
    with _record('layernorm_bwd', rows * d * x.element_size() * (3 if gate is None else 4) + 8 * rows):
        L.check(L.lib().b4c_layernorm_bwd(_p(dout), _p(x), _p(stats), _p(gamma), _p(dx), _p(dgamma), _p(dbeta), rows, d, _p(gate),
                                          gate.stride(0) if gate is not None else 0, gate_act, ws.data_ptr(),
                                          ws.numel() * ws.element_size(), dt_code(x.dtype), _st()), 'layernorm_bwd')
    return dx, dgamma, dbeta


def layernorm_bwd_add(dout, x, stats, gamma, res, into=None, dx=None, workspace=None):
    """res + backward of layernorm_fwd (b4c_layernorm_bwd_add) -> (dx, dgamma, dbeta): the input gradient of a pre-LN encoder half,
    res = the residual stream's gradient ([rows, d] view, unit column stride, 16-B aligned rows), added in fp32 before dx is
    rounded.  into = (dgamma, dbeta): fp32 [d] sinks, added to.  Fixed summation order: the same bits every launch, and with
    res == 0 the bits of layernorm_bwd."""
    rows, d = x.shape
    _cuda(dout, x, stats, gamma, res)
    if into is not None:
        dgamma, dbeta = into
    else:
        dgamma, dbeta = zeros(d, device=x.device), zeros(d, device=x.device)
    _ln_vectors(d, gamma, dgamma, dbeta)
    dx = torch.empty_like(x) if dx is None else dx
    if dout.dtype != x.dtype or dout.shape != x.shape or not dout.is_contiguous() or not x.is_contiguous() or \
            dx.dtype != x.dtype or dx.shape != x.shape or not dx.is_contiguous():
        raise B4CError('layernorm_bwd_add: dout, x and dx must be contiguous tensors of one shape and dtype')
    if stats.dtype != torch.float32 or tuple(stats.shape) != (rows, 2) or not stats.is_contiguous():
        raise B4CError('layernorm_bwd_add: stats must be the contiguous float32 [%d, 2] tensor of the forward call' % rows)
    if res.dtype != x.dtype or tuple(res.shape) != (rows, d) or res.stride(1) != 1 or \
            (res.stride(0) * res.element_size()) % 16 or res.data_ptr() % 16:
        raise B4CError('layernorm_bwd_add: res must be a [%d, %d] %s view with unit column stride' % (rows, d, x.dtype))
    if rows == 0:
        return dx, dgamma, dbeta
    ws = workspace if workspace is not None else \
        _workspace('ln_bwd', x.device, L.lib().b4c_layernorm_bwd_add_workspace_bytes(rows, d))
    with _record('layernorm_bwd_add', rows * d * x.element_size() * 4 + 8 * rows):
        L.check(L.lib().b4c_layernorm_bwd_add(_p(dout), _p(x), _p(stats), _p(gamma), _p(res), res.stride(0), _p(dx), _p(dgamma),
                                              _p(dbeta), rows, d, ws.data_ptr(), ws.numel() * ws.element_size(),
                                              dt_code(x.dtype), _st()), 'layernorm_bwd_add')
    return dx, dgamma, dbeta


def gemm_ln_bwd_supported(a, bt, n):
    """b4c_gemm_nt_ln_bwd_add takes it: bf16, at most 256 columns, 16-byte rows"""
    return a.dtype == torch.bfloat16 and bt.dtype == torch.bfloat16 and n <= 256 and n % 8 == 0 and a.shape[1] % 8 == 0 and \
        a.stride(1) == 1 and bt.stride(1) == 1 and a.stride(0) % 8 == 0 and bt.stride(0) % 8 == 0 and \
        a.data_ptr() % 16 == 0 and bt.data_ptr() % 16 == 0


def gemm_nt_ln_bwd_add(a, bt, x, stats, gamma, res, into=None, dx=None):
    """res + backward of layernorm_fwd at dout = bf16(a @ bt^T), which never reaches memory (b4c_gemm_nt_ln_bwd_add) -> (dx, dgamma,
    dbeta): gemm_nt(a, bt, n) followed by layernorm_bwd_add, up to the order of the fp32 sums.  a [M, Kp], bt [>= n, Kp] (the dX
    operand of gemm_nt), x / dx [M, n] contiguous, res an [M, n] view; bf16, n <= 256."""
    M, K = a.shape
    n = x.shape[1]
    _cuda(a, bt, x, stats, gamma, res)
    if into is not None:
        dgamma, dbeta = into
    else:
        dgamma, dbeta = zeros(n, device=x.device), zeros(n, device=x.device)
    _ln_vectors(n, gamma, dgamma, dbeta)
    dx = torch.empty_like(x) if dx is None else dx
    if not gemm_ln_bwd_supported(a, bt, n) or bt.shape[0] < n or bt.shape[1] < K:
        raise B4CError('gemm_nt_ln_bwd_add: a [M, K] and bt [>= %d, >= K] must be bf16 with 16-byte rows, K a multiple of 8, at most 256 '
                       'columns' % n)
    if x.dtype != a.dtype or x.shape[0] != M or not x.is_contiguous() or dx.dtype != x.dtype or dx.shape != x.shape or \
            not dx.is_contiguous():
        raise B4CError('gemm_nt_ln_bwd_add: x and dx must be contiguous bf16 [%d, %d] tensors' % (M, n))
    if stats.dtype != torch.float32 or tuple(stats.shape) != (M, 2) or not stats.is_contiguous():
        raise B4CError('gemm_nt_ln_bwd_add: stats must be the contiguous float32 [%d, 2] tensor of the forward call' % M)
    if res.dtype != x.dtype or tuple(res.shape) != (M, n) or res.stride(1) != 1 or (res.stride(0) * res.element_size()) % 16 or \
            res.data_ptr() % 16:
        raise B4CError('gemm_nt_ln_bwd_add: res must be a [%d, %d] %s view with unit column stride' % (M, n, x.dtype))
    if M == 0:
        return dx, dgamma, dbeta
    ws = _workspace('ln_bwd', x.device, L.lib().b4c_gemm_nt_ln_bwd_add_workspace_bytes(M, n))
    with _record('gemm_nt_ln_bwd_add', (M * K + n * K + 3 * M * n) * 2 + 8 * M, 2 * M * n * K):
        L.check(L.lib().b4c_gemm_nt_ln_bwd_add(_p(a), a.stride(0), _p(bt), bt.stride(0), _p(x), _p(stats), _p(gamma), _p(res),
                                               res.stride(0), _p(dx), _p(dgamma), _p(dbeta), M, n, K, ws.data_ptr(),
                                               ws.numel() * ws.element_size(), dt_code(x.dtype), _st()), 'gemm_nt_ln_bwd_add')
    return dx, dgamma, dbeta


def mask_positions(ids, value, cap=None, poison=None):
    """-> counts[B], offsets[B+1], flat_idx[cap], maxcount[1] (all int32, device).  More matches than `cap`: offsets stay
    within cap, maxcount comes back as -(longest row) - 1 and the int32 flag `poison` (optional) is set to -1 (include/b4c.h)."""
    _cuda(ids)
    B, S = ids.shape
    cap = B * S if cap is None else cap
    dev = ids.device
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int32, device=dev)
    flat = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    mx = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(L.lib().b4c_mask_positions(_p(ids), B, S, value, _p(counts), _p(offsets), _p(flat), cap, _p(mx), _p(poison), _st()),
            'mask_positions')
    return counts, offsets, flat, mx


def poison_rows(x, flag):
    """x (contiguous last dim) := NaN, in place, when the device flag (int32 [1]) is negative; untouched otherwise."""
    x2 = x.reshape(-1, x.shape[-1]) if x.dim() != 2 else x
    if x2.numel() and (x2.data_ptr() != x.data_ptr() or x2.stride(1) != 1):
        raise B4CError('poison_rows: needs a tensor whose leading dimensions merge into rows (got strides %s)' % (x.stride(),))
    if x2.numel() and flag is not None:
        code = 2 if x2.dtype == torch.int32 else dt_code(x2.dtype)          # B4C_I32: rows of ids, poisoned with -1
        L.check(L.lib().b4c_poison_rows(_p(x2), x2.stride(0), x2.shape[0], x2.shape[1], _p(flag), code, _st()), 'poison_rows')
    return x


def padded_index(counts, offsets, flat, B, M):
    out = torch.empty(B * M, dtype=torch.int32, device=counts.device)
    L.check(L.lib().b4c_padded_index(_p(counts), _p(offsets), _p(flat), B, M, _p(out), _st()), 'padded_index')
    return out


def gather_rows(src, idx, n_out):
    width = src.shape[1]
    out = torch.empty(n_out, width, dtype=src.dtype, device=src.device)
    if n_out == 0:
        return out
    L.check(L.lib().b4c_gather_rows(_p(src), src.stride(0), _p(idx), _p(out), width, n_out, width, dt_code(src.dtype),
                                    _st()), 'gather_rows')
    return out


def scatter_rows(src, idx, n_dst):
    n_src, width = src.shape
    if n_src == 0:
        return torch.zeros(n_dst, width, dtype=src.dtype, device=src.device)
    out = torch.empty(n_dst, width, dtype=src.dtype, device=src.device)
    L.check(L.lib().b4c_scatter_rows(_p(src), src.stride(0), _p(idx), _p(out), width, n_src, n_dst, width,
                                     dt_code(src.dtype), _st()), 'scatter_rows')
    return out


def softmax_rows(logits, V):
    """probabilities with the shape and the row pitch of `logits` ([R, W >= V]; the pad columns V .. pitch are written as 0, as include/b4c.h states)"""
    R, ld = logits.shape[0], logits.stride(0)
    probs = torch.empty(R, ld, dtype=logits.dtype, device=logits.device)
    if ld != logits.shape[1]:
        probs = probs[:, :logits.shape[1]]
    if R == 0:
        return probs
    with _record('softmax_rows', 2 * R * ld * logits.element_size()):
        L.check(L.lib().b4c_softmax_rows(_p(logits), ld, _p(probs), ld, R, V, dt_code(logits.dtype), _st()), 'softmax_rows')
    return probs


def sparse_ce_from_probs(probs, labels_f32, V, variant=L.CE_TF):
    R, ld = probs.shape[0], probs.stride(0)
    item = torch.empty(R, dtype=torch.float32, device=probs.device)
    nval = torch.zeros(1, dtype=torch.float32, device=probs.device)
    if R == 0:
        return item, nval
    L.check(L.lib().b4c_sparse_ce_from_probs(_p(probs), ld, _p(labels_f32), _p(item), _p(nval), R, V, variant,
                                             dt_code(probs.dtype), _st()), 'sparse_ce_from_probs')
    return item, nval


def softmax_ce_fwd_bwd_(logits, labels_i32, grad_scale, V, variant=L.CE_TF):
    """In place: logits -> grad_scale * dloss/dlogits.  Returns per-row loss."""
    R, ld = logits.shape[0], logits.stride(0)
    item = torch.empty(R, dtype=torch.float32, device=logits.device)
    if R == 0:
        return item
    with _record('softmax_ce', 2 * R * ld * logits.element_size()):
        L.check(L.lib().b4c_softmax_ce_fwd_bwd(_p(logits), ld, _p(labels_i32), _p(item), _p(grad_scale), R, V, variant,
                                               dt_code(logits.dtype), _st()), 'softmax_ce_fwd_bwd')
    return item


def label_scale(labels_i32, V):
    """-> fp32 [2]: 1 / n_valid (0 if no row is valid) and n_valid, valid = 0 <= label < V  (one launch)."""
    out = torch.empty(2, dtype=torch.float32, device=labels_i32.device)
    L.check(L.lib().b4c_label_scale(_p(labels_i32), labels_i32.shape[0], V, _p(out), _st()), 'label_scale')
    return out


def sum_scaled(item, scale, poison=None):
    """-> 0-dim fp32: scale[0] * sum(item) in a fixed order; NaN when the int32 flag `poison`[0] is negative."""
    out = torch.empty((), dtype=torch.float32, device=item.device)
    L.check(L.lib().b4c_sum_scaled(_p(item), item.shape[0], _p(scale), _p(poison), _p(out), _st()), 'sum_scaled')
    return out


def relu_gate(g, act):
    """g where act > 0, else 0 (same shape / dtype, contiguous, element count a multiple of 8)."""
    g, act = g.contiguous(), act.contiguous()
    out = torch.empty_like(g)
    if g.numel() == 0:
        return out
    L.check(L.lib().b4c_relu_gate(_p(g), _p(act), _p(out), g.numel(), dt_code(g.dtype), _st()), 'relu_gate')
    return out


def vocab_ce_supported(h, K):
    """The logits-free path: bf16 head input of width 64 / 128 (include/b4c.h b4c_vocab_ce_fwd)."""
    return h.dtype == torch.bfloat16 and K in (64, 128) and h.shape[1] == K


def _vce_workspace(h, R, V, K):
    return _workspace('vocab_ce', h.device, L.lib().b4c_vocab_ce_workspace_bytes(R, V, K))


def vocab_ce_fwd(h, wt, bias, labels_i32, grad_scale, V, variant=L.CE_TF):
    """h [R, K] bf16, wt [>=V, K] bf16, bias fp32 [>=V] -> (item_loss [R], dh [R, K] bf16 already scaled by
    grad_scale, rowscal [R, 8] for vocab_ce_dw).  The (R x V) logits never exist in memory."""
    _cuda(h)
    R, K = h.shape
    item = torch.empty(R, dtype=torch.float32, device=h.device)
    dh = torch.empty(R, K, dtype=h.dtype, device=h.device)
    rowscal = torch.empty(R, 8, dtype=torch.float32, device=h.device)
    if R == 0:
        return item, dh, rowscal
    ws = _vce_workspace(h, R, V, K)
    # algorithmic work: the logits GEMM and the P.W GEMM (the clipped-row sweep is data dependent and not counted)
    with _record('vocab_ce_fwd', R * K * 2 * 2 + V * K * 2, 4 * R * V * K):
        L.check(L.lib().b4c_vocab_ce_fwd(_p(h), h.stride(0), _p(wt), wt.stride(0), _p(bias), _p(labels_i32), _p(grad_scale),
                                         _p(item), _p(dh), dh.stride(0), _p(rowscal), ws.data_ptr(), ws.numel(), R, V, K,
                                         variant, _st()), 'vocab_ce_fwd')
    return item, dh, rowscal


def vocab_ce_dw(h, wt, bias, labels_i32, rowscal, V, dW, db):
    """dW [K, V] fp32 += d loss / d kernel, db [V] += d loss / d bias (second half of vocab_ce_fwd)."""
    R, K = h.shape
    if R == 0:
        return
    det = int(deterministic_vocab_dw or deterministic)
    # (the deterministic form's split partial sums: a larger workspace than the forward's)
    ws = _workspace('vocab_ce', h.device, L.lib().b4c_vocab_ce_dw_workspace_bytes(R, V, K, det))
    with _record('vocab_ce_dw', R * K * 2 + V * K * 2 + V * K * 4, 4 * R * V * K):
        L.check(L.lib().b4c_vocab_ce_dw(_p(h), h.stride(0), _p(wt), wt.stride(0), _p(bias), _p(labels_i32), _p(rowscal),
                                        _p(dW), dW.stride(0), _p(db), ws.data_ptr(), ws.numel(), R, V, K, det, _st()),
                'vocab_ce_dw')


def vocab_ce_dw_sweep(h, wt, bias, rowscal, V, dW, db, tile_begin, tile_end, background_workgroups=0):
    """the dlogit part of vocab_ce_dw for the 128-id vocabulary tiles [tile_begin, tile_end); background_workgroups > 0:
    as a background kernel of at most that many one-wave-per-SIMD workgroups (runs beside another stream's kernels)"""
    R, K = h.shape
    if R == 0 or tile_end <= tile_begin:
        return
    frac = (tile_end - tile_begin) / float((V + 127) // 128)
    with _record('vocab_ce_dw_bg' if background_workgroups > 0 else 'vocab_ce_dw',
                 int(frac * (R * K * 2 + V * K * 2 + V * K * 4)), int(frac * 4 * R * V * K)):
        L.check(L.lib().b4c_vocab_ce_dw_sweep(_p(h), h.stride(0), _p(wt), wt.stride(0), _p(bias), _p(rowscal), _p(dW), dW.stride(0),
                                              _p(db), R, V, K, tile_begin, tile_end, background_workgroups, int(deterministic_vocab_dw or deterministic), _st()),
                'vocab_ce_dw_sweep')


def vocab_ce_dw_labels(h, labels_i32, rowscal, V, dW, db):
    """the label term of vocab_ce_dw (dW[:, y] -= yd h_row, db[y] -= yd)"""
    R, K = h.shape
    if R == 0:
        return
    ws = _vce_workspace(h, R, V, K)
    L.check(L.lib().b4c_vocab_ce_dw_labels(_p(h), h.stride(0), _p(labels_i32), _p(rowscal), _p(dW), dW.stride(0), _p(db),
                                           ws.data_ptr(), ws.numel(), R, V, K, int(deterministic_vocab_dw or deterministic), _st()), 'vocab_ce_dw_labels')


fused_softmax_proj = True      # Dense(V, softmax) of the bf16 path in one pass over (R x V): lse sweep + softmax epilogue


def vocab_softmax(h, wt, bias, Np, V):
    """probs [R, Np] (bf16, row_pitch(Np) pitch) = softmax over the first V columns of h wt^T + bias; columns V.. are 0.
    The logits never reach HBM: b4c_vocab_lse recomputes them for the row lse, b4c_gemm_nt_softmax writes probabilities."""
    R, K = h.shape
    probs = empty_rows(R, Np, h.dtype, h.device)
    if R == 0:
        return probs
    ws = _vce_workspace(h, R, V, K)
    lse2 = torch.empty(R, dtype=torch.float32, device=h.device)
    with _record('vocab_lse', R * K * 2 + V * K * 2, 2 * R * V * K):
        L.check(L.lib().b4c_vocab_lse(_p(h), h.stride(0), _p(wt), wt.stride(0), _p(bias), _p(lse2), ws.data_ptr(), ws.numel(),
                                      R, V, K, _st()), 'vocab_lse')
    with _record('vocab_proj', R * K * 2 + Np * K * 2 + R * Np * 2, 2 * R * Np * K):
        L.check(L.lib().b4c_gemm_nt_softmax(_p(h), h.stride(0), _p(wt), wt.stride(0), _p(probs), probs.stride(0), R, Np, K,
                                            _p(bias), _p(lse2), _st()), 'gemm_nt_softmax')
    if Np != V:
        probs[:, V:].zero_()
    return probs


fused_rank = True      # bf16 scoring path: ranks / top-k ids without the (R x V) scores in memory (b4c_vocab_rank, b4c_vocab_topk)


def _rank_workspace(h, R, V, K):
    return _workspace('vocab_rank', h.device, L.lib().b4c_vocab_rank_workspace_bytes(R, V, K))


def exclusions(ex, V, labels=None):
    """-> int32 [R, E] device tensor: the canonical per-row exclusion lists every `exclude=` of the ranking entry points takes
    (b4c_exclusions_prep: the ids of [0, V) other than the row's label, ascending, no duplicates, then -1).
    ex: an integer tensor [R, E] (negative entries: padding; out-of-range ids and duplicates are ignored) or a host list of R
    lists of ids.  labels (int [R], optional): a row's label is never excluded.  E <= MAX_EXCL."""
    if isinstance(ex, torch.Tensor):
        if ex.dim() != 2:
            raise B4CError('exclusions: an [R, E] tensor of item ids is needed, got shape %s' % (tuple(ex.shape),))
        if ex.dtype.is_floating_point or ex.dtype.is_complex or ex.dtype == torch.bool:
            raise B4CError('exclusions: item ids must be an integer tensor, got %s' % ex.dtype)
        t = ex
    else:
        rows = [list(r) for r in ex]
        E = max([len(r) for r in rows] + [0])
        t = torch.full((len(rows), E), -1, dtype=torch.int64)
        for i, r in enumerate(rows):
            if r:
                t[i, :len(r)] = torch.as_tensor(r, dtype=torch.int64)
    R, E = t.shape
    if E > L.MAX_EXCL:
        raise B4CError('exclusions: %d ids per row; at most %d (B4C_MAX_EXCL)' % (E, L.MAX_EXCL))
    if t.dtype != torch.int32:          # ids outside the int32 range cannot be items: mark them out of range before narrowing
        t = torch.where((t >= 0) & (t < V), t, torch.full_like(t, -1)).to(torch.int32)
    dev = t.device if t.is_cuda else (labels.device if isinstance(labels, torch.Tensor) and labels.is_cuda else torch.device('cuda'))
    t = t.to(dev).contiguous()
    lab = None
    if labels is not None:
        lab = torch.as_tensor(labels, device=dev).reshape(-1).to(torch.int32).contiguous()
        if lab.shape[0] != R:
            raise B4CError('exclusions: %d labels for %d rows' % (lab.shape[0], R))
    out = torch.empty(R, E, dtype=torch.int32, device=dev)
    if R and E:
        L.check(L.lib().b4c_exclusions_prep(_p(t), t.stride(0), R, E, V, _p(lab), _p(out), _st()), 'exclusions_prep')
    return out


def _excl_args(exclude, R, who):
    """(pointer, ld, E) of a canonical exclusion tensor (ops.exclusions) for R rows"""
    if not isinstance(exclude, torch.Tensor) or exclude.dim() != 2 or exclude.dtype != torch.int32 or not exclude.is_cuda:
        raise B4CError('%s: exclude must be the int32 [R, E] device tensor of ops.exclusions' % who)
    if exclude.shape[0] != R or (exclude.shape[1] and exclude.stride(1) != 1):
        raise B4CError('%s: exclude has %d rows (contiguous ids) for %d rows' % (who, exclude.shape[0], R))
    if R > 1 and exclude.shape[1] and exclude.stride(0) < exclude.shape[1]:      # (rows that overlap: not ops.exclusions' own)
        raise B4CError('%s: exclude rows overlap in memory (stride %d < %d ids); pass ops.exclusions(...)'
                       % (who, exclude.stride(0), exclude.shape[1]))
    return _p(exclude), max(exclude.stride(0), exclude.shape[1]), exclude.shape[1]


def _excl_entry(who, exclude, R):
    """(name, trailing arguments) of the entry point `who` serves a call through: `who` itself and none without a list, the
    _excl one and the list's (pointer, ld, E) with one; the name is also the label of the call's status check"""
    if exclude is None:
        return who, ()
    return who + '_excl', _excl_args(exclude, R, who)


def vocab_rank(h, wt, bias, labels_i32, V, exclude=None):
    """rank [R] int32 of the label among the V scores h wt^T + bias (items ranked before it; ties -> lower index first;
    negative: no valid label).  The scores never exist in memory.  exclude (ops.exclusions): items of a row's list do not
    count (b4c_vocab_rank_excl)."""
    _cuda(h)
    R, K = h.shape
    rank = torch.empty(R, dtype=torch.int32, device=h.device)
    name, ex = _excl_entry('vocab_rank', exclude, R)
    if R == 0:
        return rank
    ws = _rank_workspace(h, R, V, K)
    with _record('vocab_rank', R * K * 2 + V * K * 2, 2 * R * V * K):
        L.check(getattr(L.lib(), 'b4c_' + name)(_p(h), h.stride(0), _p(wt), wt.stride(0), _p(bias), _p(labels_i32), _p(rank),
                                                ws.data_ptr(), ws.numel(), R, V, K, *ex, _st()), name)
    return rank


def rank_metrics(rank, k):
    """-> (hit [R], ndcg [R]) fp32: [rank < k], [rank < k] / log2(rank + 2); rows with a negative rank: 0"""
    R = rank.shape[0]
    hit = torch.empty(R, dtype=torch.float32, device=rank.device)
    ndcg = torch.empty(R, dtype=torch.float32, device=rank.device)
    if R:
        L.check(L.lib().b4c_rank_metrics(_p(rank), R, k, _p(hit), _p(ndcg), _st()), 'rank_metrics')
    return hit, ndcg


def vocab_topk(h, wt, bias, V, k, labels_i32=None, exclude=None):
    """-> (idx [R, k] int32, hit, ndcg (when labels are given), overflow int32 [1]): the k best item ids of every row of
    h wt^T + bias in order, scores never in memory.  overflow[0] rows (ids -1) have too many ties at the selection
    threshold: rank those on materialised scores.  exclude (ops.exclusions): a row's listed items are left out
    (b4c_vocab_topk_excl; ids -1 past the items that remain)."""
    _cuda(h)
    R, K = h.shape
    name, ex = _excl_entry('vocab_topk', exclude, R)
    idx = torch.empty(R, k, dtype=torch.int32, device=h.device)
    hit = torch.empty(R, dtype=torch.float32, device=h.device) if labels_i32 is not None else None
    ndcg = torch.empty(R, dtype=torch.float32, device=h.device) if labels_i32 is not None else None
    overflow = torch.empty(1, dtype=torch.int32, device=h.device)
    if R == 0:
        return idx, hit, ndcg, overflow.zero_()
    ws = _rank_workspace(h, R, V, K)
    with _record('vocab_topk', 2 * (R * K * 2 + V * K * 2), 4 * R * V * K):
        L.check(getattr(L.lib(), 'b4c_' + name)(_p(h), h.stride(0), _p(wt), wt.stride(0), _p(bias), k, _p(idx), _p(labels_i32),
                                                _p(hit), _p(ndcg), _p(overflow), ws.data_ptr(), ws.numel(), R, V, K, *ex, _st()),
                name)
    return idx, hit, ndcg, overflow


class VocabSoftmaxFn(torch.autograd.Function):
    """Dense(V, softmax) (head.py:36) on the head's trunk output, probabilities materialised once, logits never:
    apply(h [R, K] bf16, pack, V, kernel, bias) -> probs [R, Np].  Backward: the softmax Jacobian on the saved
    probabilities (b4c_softmax_rows_bwd), then the projection's dW / db / dh as MLPFn does."""

    @staticmethod
    def forward(ctx, h, pack, V, kernel, bias):
        h = h.contiguous()
        training = any(ctx.needs_input_grad)       # (grad mode is off inside forward: ask what autograd will want)
        wt, _, b = pack.get(h.dtype, h.shape[1], training)
        probs = vocab_softmax(h, wt, b, pack.Np, V)
        if training:
            ctx.save_for_backward(h, probs)
            ctx.pack, ctx.V, ctx.params = pack, V, (kernel, bias)
        return probs

    @staticmethod
    def backward(ctx, g):
        h, probs = ctx.saved_tensors
        pack = ctx.pack
        kernel, bias = ctx.params
        g = _rows_ok(g, probs.dtype)
        dlogits = softmax_rows_bwd(probs, g, ctx.V)
        _, wc, _ = pack.get(h.dtype, h.shape[1], True)
        actx, sinks = grad_sinks(kernel, bias)
        queue_dw(actx, h, dlogits, pack.K, pack.N, sinks[:1], sinks[1:], (kernel, bias))
        with _timed('vocab_proj_dx'):
            dh = gemm_nt(dlogits, wc, h.shape[1])
        flush_pending_dw(actx)
        return sink_returns(ctx, (dh, None, None), actx, sinks)


topk_threshold = True     # threshold-selection kernel (one HBM read per row); False: per-thread sorted lists only


def topk_rows(scores, V, k, labels_i32=None, exclude=None):
    """-> (idx [R, k] int32, hit, ndcg) of materialised scores [R, >= V] (fp32 / bf16).  exclude (ops.exclusions): a row's
    listed items are left out (b4c_topk_rows_excl); `scores` is only read."""
    _cuda(scores)
    R, ld = scores.shape[0], scores.stride(0)
    name, ex = _excl_entry('topk_rows', exclude, R)
    idx = torch.empty(R, k, dtype=torch.int32, device=scores.device)
    hit = torch.empty(R, dtype=torch.float32, device=scores.device) if labels_i32 is not None else None
    ndcg = torch.empty(R, dtype=torch.float32, device=scores.device) if labels_i32 is not None else None
    if R == 0:
        return idx, hit, ndcg
    redo = torch.empty(R, dtype=torch.int32, device=scores.device) if topk_threshold else None
    fn = L.lib().b4c_topk_rows_excl if ex else L.lib().b4c_topk_rows_ws
    with _record('topk_rows', R * ld * scores.element_size()):
        L.check(fn(_p(scores), ld, R, V, k, _p(idx), _p(labels_i32), _p(hit), _p(ndcg), _p(redo), dt_code(scores.dtype), *ex, _st()),
                name)
    return idx, hit, ndcg


# ---- candidate lists (include/b4c.h "candidate lists"): sampled negatives, scores / rank / top-k of a per-row list of items ----
def _cand_args(cand, R, who):
    """(tensor, ld, C) of an int32 [R, C] device candidate tensor.  Rows that overlap in memory (a list shared by every row
    through expand(R, -1): stride(0) == 0) are copied out first: the kernels address row r at r * ld with ld >= C."""
    if not isinstance(cand, torch.Tensor) or cand.dim() != 2 or cand.dtype != torch.int32:
        raise B4CError('%s: candidates must be an int32 [R, C] tensor of item ids' % who)
    if cand.shape[0] != R:
        raise B4CError('%s: candidates have %d rows for %d rows' % (who, cand.shape[0], R))
    C = cand.shape[1]
    if not 1 <= C <= L.MAX_CAND:
        raise B4CError('%s: %d candidates per row; 1 .. %d (B4C_MAX_CAND)' % (who, C, L.MAX_CAND))
    if R and cand.stride(1) != 1:
        raise B4CError('%s: candidate ids must be contiguous within a row' % who)
    if R > 1 and cand.stride(0) < C:
        cand = cand.contiguous()
    return cand, max(cand.stride(0), C), C


def _cand_labels(labels, R, who):
    if labels is None:
        return None
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or labels.numel() != R:
        raise B4CError('%s: labels must be an int32 tensor of %d ids' % (who, R))
    return labels.reshape(-1).contiguous()


def _cand_k(k, who):
    if not 0 <= int(k) <= L.MAX_TOPK:
        raise B4CError('%s: k = %d (0 .. %d)' % (who, k, L.MAX_TOPK))
    return int(k)


def sample_candidates(labels, V, num_negatives, seed, row_base=0, exclude=None, item_cdf=None):
    """-> (cand int32 [R, 1 + N], short int32 [1]) (b4c_sample_candidates): cand[r][0] = labels[r], then N distinct negatives
    of [0, V) in acceptance order -- never the label, never an item of the row's exclusion list.  Attempt j of row r draws
    x = b4c_rand64(seed, ((row_base + r) << 20) | j): uniform (item_cdf None) mulhi64(x, V), or popularity (item_cdf: int64 [V]
    inclusive prefix sum of per-item counts, total = item_cdf[-1] > 0) min{i : item_cdf[i] > mulhi64(x, total)}.  After 64 N
    attempts a row still short keeps -1 in its tail and is counted in short[0]; rows without a valid label are -1 throughout.
    exclude: ops.exclusions lists, one per row.  A pure function of (seed, row_base + r, labels, exclusions, item_cdf).
    The total of item_cdf is not read back (no stream synchronisation here): a cdf whose total is <= 0 draws nothing, and every
    row with a valid label comes back short.  cloze.sample_candidates checks the counts on the host, where it builds the cdf."""
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.dtype != torch.int32:
        raise B4CError('sample_candidates: labels must be an int32 [R] tensor')
    R, V, N = labels.shape[0], int(V), int(num_negatives)
    if V <= 0 or not 0 <= N < L.MAX_CAND:
        raise B4CError('sample_candidates: V = %d, num_negatives = %d (0 .. %d)' % (V, N, L.MAX_CAND - 1))
    if not 0 <= int(row_base) < (1 << 44) or not 0 <= int(seed) < (1 << 64):
        raise B4CError('sample_candidates: row_base %d (0 .. 2^44) / seed %d (0 .. 2^64)' % (row_base, seed))
    ex, ld_e, E = _excl_args(exclude, R, 'sample_candidates') if exclude is not None else (None, 0, 0)
    if item_cdf is not None:
        if not isinstance(item_cdf, torch.Tensor) or item_cdf.dtype != torch.int64 or item_cdf.dim() != 1 or item_cdf.shape[0] != V:
            raise B4CError('sample_candidates: item_cdf must be an int64 [V] = [%d] prefix sum of item counts' % V)
        item_cdf = item_cdf.contiguous()      # (its total is not read back here: a cdf without mass draws nothing, rows short)
    _cuda(labels, item_cdf)
    labels = labels.contiguous()
    cand = torch.empty(R, N + 1, dtype=torch.int32, device=labels.device)
    short = torch.empty(1, dtype=torch.int32, device=labels.device)
    with _record('sample_candidates', R * (N + 1) * 4 + R * E * 4):
        L.check(L.lib().b4c_sample_candidates(_p(labels), R, V, N, int(seed), int(row_base), ex, ld_e, E, _p(item_cdf), _p(cand),
                                              N + 1, _p(short), _st()), 'sample_candidates')
    return cand, short


def candidate_scores(h, wt, bias, cand, V, labels=None, k=0, want_scores=True):
    """-> (scores fp32 [R, C] or None, rank int32 [R] or None, idx int32 [R, k] or None) of a per-row candidate list
    (b4c_candidate_score): s(r, c) = h[r] . wt[c] + bias[c] (fp32 accumulation); NaN where cand[r][p] is absent (< 0 or >= V).
    rank (labels int32 [R] given): distinct listed items other than the label that score above it, or equal and with a lower id
    (negative: no valid label).  idx (k > 0): the k best distinct listed items, ties -> lower id, -1 past the last.
    h [R, K] and wt [>= V, >= K] bf16 or fp32 (one dtype), K % 8 == 0, K <= 1024; bias fp32 [>= V]."""
    if not isinstance(h, torch.Tensor) or h.dim() != 2:
        raise B4CError('candidate_scores: h must be an [R, K] tensor')
    R, K = h.shape
    dt = dt_code(h.dtype)
    if K % 8 or not 8 <= K <= 1024 or h.stride(1) != 1:
        raise B4CError('candidate_scores: K = %d (a multiple of 8, 8 .. 1024, contiguous rows)' % K)
    if (not isinstance(wt, torch.Tensor) or wt.dim() != 2 or wt.dtype != h.dtype or wt.shape[0] < V or wt.shape[1] < K
            or wt.stride(1) != 1 or wt.stride(0) % 8):
        raise B4CError('candidate_scores: wt must be [>= V, >= K] in h\'s dtype with a pitch that is a multiple of 8')
    if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or bias.numel() < V:
        raise B4CError('candidate_scores: bias must be fp32 [>= V]')
    cand, ld_c, C = _cand_args(cand, R, 'candidate_scores')
    k = _cand_k(k, 'candidate_scores')
    lab = _cand_labels(labels, R, 'candidate_scores')
    _cuda(h, wt, bias, cand, lab)
    dev = h.device
    scores = torch.empty(R, C, dtype=torch.float32, device=dev) if want_scores else None
    rank = torch.empty(R, dtype=torch.int32, device=dev) if lab is not None else None
    idx = torch.empty(R, k, dtype=torch.int32, device=dev) if k else None
    if R == 0:
        return scores, rank, idx
    es, Kp = h.element_size(), wt.shape[1]
    with _record('candidate_score', R * K * es + R * C * Kp * es + R * C * 4, 2 * R * C * K):
        L.check(L.lib().b4c_candidate_score(_p(h), h.stride(0), _p(wt), wt.stride(0), _p(bias.contiguous()), _p(cand), ld_c, R, C, V, K,
                                            dt, _p(lab), _p(scores), C, _p(rank), k, _p(idx), _st()), 'candidate_score')
    return scores, rank, idx


def candidate_rank_rows(scores, V, cand, labels=None, k=0):
    """-> (rank, idx) of candidate_scores' definition on MATERIALISED scores [R, >= V] (fp32 probabilities or logits, bf16
    logits) (b4c_candidate_rank_rows): the listed columns are gathered, `scores` is only read."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2 or scores.shape[1] < V or scores.stride(1) != 1:
        raise B4CError('candidate_rank_rows: scores must be an [R, >= V] tensor with contiguous rows')
    dt = dt_code(scores.dtype)
    R = scores.shape[0]
    cand, ld_c, C = _cand_args(cand, R, 'candidate_rank_rows')
    k = _cand_k(k, 'candidate_rank_rows')
    lab = _cand_labels(labels, R, 'candidate_rank_rows')
    _cuda(scores, cand, lab)
    rank = torch.empty(R, dtype=torch.int32, device=scores.device) if lab is not None else None
    idx = torch.empty(R, k, dtype=torch.int32, device=scores.device) if k else None
    if R == 0:
        return rank, idx
    with _record('candidate_rank_rows', R * C * (scores.element_size() + 4)):
        L.check(L.lib().b4c_candidate_rank_rows(_p(scores), scores.stride(0), dt, _p(cand), ld_c, R, C, V, _p(lab), _p(rank), k, _p(idx),
                                                _st()), 'candidate_rank_rows')
    return rank, idx


CAND_LOSS_KINDS = {'bce': L.CAND_BCE, 'softmax': L.CAND_SOFTMAX}


def _cand_loss_args(who, h, table, row_off, V, cand):
    """the operand checks candidate_loss_fwd and candidate_loss_bwd share -> (cand, ld_c, C, R, K, dtype code)"""
    if not isinstance(h, torch.Tensor) or h.dim() != 2:
        raise B4CError('%s: h must be an [R, K] tensor' % who)
    R, K = h.shape
    dt = dt_code(h.dtype)
    if K % 8 or not 8 <= K <= 1024 or h.stride(1) != 1 or h.stride(0) % 8:
        raise B4CError('%s: K = %d (a multiple of 8, 8 .. 1024, contiguous rows with a pitch that is a multiple of 8)' % (who, K))
    if (not isinstance(table, torch.Tensor) or table.dim() != 2 or table.dtype != torch.float32 or table.shape[1] < K
            or table.stride(1) != 1 or table.stride(0) % 4):
        raise B4CError('%s: table must be the fp32 master table [rows, >= K] with a pitch that is a multiple of 4' % who)
    if not 0 <= int(row_off) <= table.shape[0] - V:
        raise B4CError('%s: rows %d .. %d of a table of %d rows' % (who, row_off, row_off + V, table.shape[0]))
    cand, ld_c, C = _cand_args(cand, R, who)
    return cand, ld_c, C, R, K, dt


def candidate_loss_fwd(h, table, bias, cand, V, kind, row_off=0, want_scores=False):
    """-> (item_loss fp32 [R], g fp32 [R, C], scores fp32 [R, C] or None) of each row's own candidate list, target in column 0
    (b4c_candidate_loss_fwd, include/b4c.h): kind 'bce' = softplus(-s_0) + sum of softplus(s_c) over the other present
    entries, 'softmax' = logsumexp over the present entries - s_0; g the loss's derivative by each score.  An entry < 0 or >= V is
    absent (g = 0); a row whose column 0 is absent is ignored (loss 0, g = 0).  s = h . table[row_off + id] + bias[id] in fp32;
    for bf16 h the table's elements are rounded to bf16 first.  h [R, K] bf16 or fp32, table the fp32 master [rows, >= K]."""
    if kind not in CAND_LOSS_KINDS:
        raise B4CError("candidate_loss_fwd: kind %r ('bce' or 'softmax')" % (kind,))
    cand, ld_c, C, R, K, dt = _cand_loss_args('candidate_loss_fwd', h, table, row_off, V, cand)
    if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or bias.numel() < V:
        raise B4CError('candidate_loss_fwd: bias must be fp32 [>= V]')
    _cuda(h, table, bias, cand)
    dev = h.device
    item = torch.empty(R, dtype=torch.float32, device=dev)
    g = torch.empty(R, C, dtype=torch.float32, device=dev)
    scores = torch.empty(R, C, dtype=torch.float32, device=dev) if want_scores else None
    if R == 0:
        return item, g, scores
    with _record('candidate_loss_fwd', R * K * h.element_size() + R * C * (K * 4 + 12), 2 * R * C * K):
        L.check(L.lib().b4c_candidate_loss_fwd(_p(h), h.stride(0), _p(table), table.stride(0), table.shape[0], int(row_off),
                                               _p(bias.contiguous()), _p(cand), ld_c, R, C, V, K, dt, CAND_LOSS_KINDS[kind], _p(item),
                                               _p(g), C, _p(scores), C, _st()), 'candidate_loss_fwd')
    return item, g, scores


CANDX_LOSS_KINDS = {'bce': L.CANDX_BCE, 'softmax': L.CANDX_SOFTMAX, 'bpr': L.CANDX_BPR}


def candidate_loss_fwd_ex(h, table, bias, cand, V, kind, row_off=0, want_scores=False, beta=1.0, corr=None, correct_target=False):
    """candidate_loss_fwd with the additions of include/b4c.h (b4c_candidate_loss_fwd_ex) -> (item_loss, g, scores or
    None).  kind 'bce' = beta * softplus(-z_0) + sum of softplus(z_c) (beta finite, >= 0; 1.0: SASRec's, another value: gSASRec's
    gBCE), 'softmax' as there, 'bpr' = sum over the present negatives of softplus(z_c - z_0).  z = s - corr[id] at every present
    negative, and at the target too with correct_target (corr fp32 [>= V], e.g. cloze.log_expected_count: the logQ correction);
    corr None: z = s.  scores are the uncorrected s; g is the derivative by z and by s alike, candidate_loss_bwd takes it as it is.
    With 'bce' / 'softmax', beta 1.0 and no corr the result is bit for bit candidate_loss_fwd's."""
    who = 'candidate_loss_fwd_ex'
    if kind not in CANDX_LOSS_KINDS:
        raise B4CError("%s: kind %r ('bce', 'softmax' or 'bpr')" % (who, kind))
    try:
        beta = float(beta)
    except (TypeError, ValueError):
        raise B4CError('%s: beta = %r (a finite number >= 0)' % (who, beta)) from None
    if not (0.0 <= beta < float('inf')):
        raise B4CError('%s: beta = %r (a finite number >= 0)' % (who, beta))
    if corr is None and correct_target:
        raise B4CError('%s: correct_target needs corr (there is no correction to apply to the target)' % who)
    cand, ld_c, C, R, K, dt = _cand_loss_args(who, h, table, row_off, V, cand)
    if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or bias.numel() < V:
        raise B4CError('%s: bias must be fp32 [>= V]' % who)
    if corr is not None and (not isinstance(corr, torch.Tensor) or corr.dtype != torch.float32 or corr.dim() != 1 or corr.numel() < V
                             or not corr.is_contiguous()):
        raise B4CError('%s: corr must be a contiguous fp32 [>= V] tensor' % who)
    _cuda(h, table, bias, cand, *(() if corr is None else (corr,)))
    dev = h.device
    item = torch.empty(R, dtype=torch.float32, device=dev)
    g = torch.empty(R, C, dtype=torch.float32, device=dev)
    scores = torch.empty(R, C, dtype=torch.float32, device=dev) if want_scores else None
    if R == 0:
        return item, g, scores
    flags = L.CANDX_CORR_TARGET if correct_target else 0
    with _record(who, R * K * h.element_size() + R * C * (K * 4 + (12 if corr is None else 16)), 2 * R * C * K):
        L.check(L.lib().b4c_candidate_loss_fwd_ex(_p(h), h.stride(0), _p(table), table.stride(0), table.shape[0], int(row_off),
                                                  _p(bias.contiguous()), _p(cand), ld_c, R, C, V, K, dt, CANDX_LOSS_KINDS[kind], beta,
                                                  _p(corr), flags, _p(item), _p(g), C, _p(scores), C, _st()), who)
    return item, g, scores


def candidate_loss_bwd(h, table, cand, g, gscale, V, dtable, dbias, row_off=0):
    """-> dh [R, K] in h's dtype = gscale * sum_c g[r][c] * table[row_off + cand[r][c]], and ADDS gscale * g[r][c] * h[r] into row
    row_off + cand[r][c] of dtable (fp32, the table's shape) and gscale * g[r][c] into dbias[cand[r][c]] (fp32 [>= V]) with float
    atomics (b4c_candidate_loss_bwd).  g [R, C] from candidate_loss_fwd, gscale a device fp32 [1]."""
    who = 'candidate_loss_bwd'
    cand, ld_c, C, R, K, dt = _cand_loss_args(who, h, table, row_off, V, cand)
    if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.shape != (R, C) or (R and g.stride(1) != 1):
        raise B4CError('%s: g must be the fp32 [R, C] = [%d, %d] coefficients of candidate_loss_fwd' % (who, R, C))
    if not isinstance(gscale, torch.Tensor) or gscale.dtype != torch.float32 or gscale.numel() != 1:
        raise B4CError('%s: gscale must be a device fp32 tensor of one element' % who)
    if (not isinstance(dtable, torch.Tensor) or dtable.dtype != torch.float32 or dtable.shape != table.shape
            or not dtable.is_contiguous()):
        raise B4CError('%s: dtable must be a contiguous fp32 tensor of the table\'s shape' % who)
    if not isinstance(dbias, torch.Tensor) or dbias.dtype != torch.float32 or dbias.numel() < V or not dbias.is_contiguous():
        raise B4CError('%s: dbias must be contiguous fp32 [>= V]' % who)
    _cuda(h, table, cand, g, gscale, dtable, dbias)
    dh = torch.empty(R, K, dtype=h.dtype, device=h.device)
    if R == 0:
        return dh
    with _record('candidate_loss_bwd', R * K * h.element_size() * 2 + R * C * (K * 8 + 12), 4 * R * C * K):
        L.check(L.lib().b4c_candidate_loss_bwd(_p(h), h.stride(0), _p(table), table.stride(0), table.shape[0], int(row_off), _p(cand),
                                               ld_c, _p(g), max(g.stride(0), C), _p(gscale), R, C, V, K, dt, _p(dh), K, _p(dtable),
                                               dtable.stride(0), _p(dbias), _st()), 'candidate_loss_bwd')
    return dh


# ---- in-batch contrastive loss (include/b4c.h): NT-Xent / InfoNCE over the rows of a batch ----
NCE_SIMILARITIES = ('dot', 'cos')


def _nce_args(who, z, pos, group, temperature, similarity):
    """the operand checks nce_fwd and nce_bwd share -> (pos, group or None, N, K, dtype code, inv_temp, flags)"""
    if not isinstance(z, torch.Tensor) or z.dim() != 2:
        raise B4CError('%s: z must be an [N, K] tensor' % who)
    N, K = z.shape
    dt = dt_code(z.dtype)
    per16 = 16 // z.element_size()
    if K % 8 or not 8 <= K <= 128 or z.stride(1) != 1 or z.stride(0) % per16 or z.stride(0) < K or z.data_ptr() % 16:
        raise B4CError('%s: K = %d (a multiple of 8, 8 .. 128, contiguous 16-byte aligned rows)' % (who, K))
    if N >= L.NCE_MAX_N:
        raise B4CError('%s: N = %d rows (below 2^24)' % (who, N))
    if similarity not in NCE_SIMILARITIES:
        raise B4CError("%s: similarity %r ('dot' or 'cos')" % (who, similarity))
    try:
        t = float(temperature)
    except (TypeError, ValueError):
        raise B4CError('%s: temperature = %r (a finite number > 0)' % (who, temperature)) from None
    if not (0.0 < t < float('inf')) or not (0.0 < 1.0 / t < 3.0e38):
        raise B4CError('%s: temperature = %r (a finite number > 0 whose inverse is a finite float)' % (who, temperature))
    if not isinstance(pos, torch.Tensor) or pos.dtype != torch.int32 or pos.shape != (N,):
        raise B4CError('%s: pos must be an int32 [N] = [%d] tensor (the row of each row\'s positive; out of range or itself: ignored)'
                       % (who, N))
    if group is not None and (not isinstance(group, torch.Tensor) or group.dtype != torch.int32 or group.shape != (N,)):
        raise B4CError('%s: group must be None or an int32 [N] = [%d] tensor (negative: none)' % (who, N))
    _cuda(z, pos, group)
    return pos.contiguous(), (None if group is None else group.contiguous()), N, K, dt, 1.0 / t, (L.NCE_COSINE if similarity == 'cos' else 0)


def nce_fwd(z, pos, group=None, temperature=1.0, similarity='dot'):
    """-> (item_loss fp32 [N], lse fp32 [N], rnorm fp32 [N] or None) of the in-batch contrastive loss (b4c_nce_fwd, include/b4c.h):
    row i is a query when pos[i] names another row of the batch; its keys are that positive and every other query row, except (group
    given) rows of its own non-negative group; item_loss[i] = logsumexp over the keys of s_ij - s_{i, pos[i]}, s = z_i . z_j /
    temperature ('dot') or the cosine of the two rows / temperature ('cos': rnorm comes back, 1 / max(||z_i||, 1e-12)).  Other rows:
    0.  z [N, K] bf16 or fp32, K % 8 == 0, 8 .. 128.  The [N, N] scores never reach memory."""
    who = 'nce_fwd'
    pos, group, N, K, dt, inv_t, flags = _nce_args(who, z, pos, group, temperature, similarity)
    dev = z.device
    item = torch.empty(N, dtype=torch.float32, device=dev)
    lse = torch.empty(N, dtype=torch.float32, device=dev)
    rnorm = torch.empty(N, dtype=torch.float32, device=dev) if flags else None
    if N == 0:
        return item, lse, rnorm
    with _record(who, N * K * z.element_size() * (1 + (N + 127) // 128) + N * 24, 2 * N * N * K):
        L.check(L.lib().b4c_nce_fwd(_p(z), z.stride(0), N, K, dt, _p(pos), _p(group), inv_t, flags, _p(rnorm), _p(lse), _p(item), _st()), who)
    return item, lse, rnorm


def nce_bwd(z, pos, group, temperature, similarity, rnorm, lse, gscale):
    """-> dz [N, K] in z's dtype: gscale[0] times the derivative of the sum of nce_fwd's item_loss by z (b4c_nce_bwd), written, not
    accumulated.  lse, rnorm: nce_fwd's (rnorm None for 'dot'); gscale a device fp32 [1].  One sweep over the score tiles serves
    a row's own loss and its part in every other row's."""
    who = 'nce_bwd'
    pos, group, N, K, dt, inv_t, flags = _nce_args(who, z, pos, group, temperature, similarity)
    if not isinstance(lse, torch.Tensor) or lse.dtype != torch.float32 or lse.shape != (N,) or not lse.is_contiguous():
        raise B4CError('%s: lse must be the contiguous fp32 [N] = [%d] of nce_fwd' % (who, N))
    if flags and (not isinstance(rnorm, torch.Tensor) or rnorm.dtype != torch.float32 or rnorm.shape != (N,) or not rnorm.is_contiguous()):
        raise B4CError("%s: similarity 'cos' needs the contiguous fp32 [N] = [%d] rnorm of nce_fwd" % (who, N))
    if not isinstance(gscale, torch.Tensor) or gscale.dtype != torch.float32 or gscale.numel() != 1:
        raise B4CError('%s: gscale must be a device fp32 tensor of one element' % who)
    _cuda(lse, gscale, rnorm if flags else None)
    dz = torch.empty(N, K, dtype=z.dtype, device=z.device)
    if N == 0:
        return dz
    with _record(who, N * K * z.element_size() * (2 + (N + 127) // 128) + N * 28, 4 * N * N * K):
        L.check(L.lib().b4c_nce_bwd(_p(z), z.stride(0), N, K, dt, _p(pos), _p(group), inv_t, flags, _p(rnorm) if flags else None, _p(lse),
                                    _p(gscale), _p(dz), K, _st()), who)
    return dz


# ---- Cloze batches (include/b4c.h "Cloze batches"): model inputs and padded labels from a CSR data set on the device ----
CLOZE_TRAIN, CLOZE_EVAL = 0, 1
CLOZE_MAX_WIDTH, CLOZE_MAX_LABELS = L.MAX_BATCH_WIDTH, L.MAX_CLOZE_LABELS


# what the batch builders (Cloze, next-item, side features) check alike; `who` names the caller in the message
def _csr_pair(who, items, offsets):
    """the data set -> (items, offsets), contiguous"""
    if not isinstance(items, torch.Tensor) or items.dim() != 1 or items.dtype != torch.int32:
        raise B4CError('%s: items must be an int32 [N] tensor of item indices' % who)
    if not isinstance(offsets, torch.Tensor) or offsets.dim() != 1 or offsets.dtype != torch.int64 or offsets.shape[0] < 1:
        raise B4CError('%s: offsets must be an int64 [n_seq + 1] tensor' % who)
    return items.contiguous(), offsets.contiguous()


def _window_table(who, win_seq, win_start, win_len, read=True):
    """the device window table -> its three tensors, contiguous; (None, None, None) for a layout that does not read it"""
    if not read:
        return None, None, None
    for name, t in (('win_seq', win_seq), ('win_start', win_start), ('win_len', win_len)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.int32 or t.shape[0] != win_seq.shape[0]:
            raise B4CError('%s: %s must be an int32 [n_win] tensor (win_seq, win_start, win_len: one length)' % (who, name))
    return win_seq.contiguous(), win_start.contiguous(), win_len.contiguous()


def _row_index(who, name, t, what, B=None, optional=False):
    """seq_idx / row_win: what every batch row names -> contiguous; None where optional (row b names b)"""
    if t is None and optional:
        return None
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.int32 or (B is not None and t.shape[0] != B):
        raise B4CError('%s: %s must be an int32 [B]%s tensor of %s%s' % (who, name, '' if B is None else ' = [%d]' % B, what,
                                                                     ', or None' if optional else ''))
    return t.contiguous()


def _batch_width(who, W):
    if not 1 <= int(W) <= CLOZE_MAX_WIDTH:
        raise B4CError('%s: W = %d (1 .. %d)' % (who, W, CLOZE_MAX_WIDTH))
    return int(W)


def _holdout_args(who, holdout, max_len, least, max_len_read):
    """-> (holdout, max_len): holdout / drop >= least (None: the layout does not read it), max_len (None: the width limit) >= 1
    where the layout reads it"""
    holdout, max_len = int(holdout), CLOZE_MAX_WIDTH if max_len is None else int(max_len)
    if (least is not None and holdout < least) or (max_len_read and max_len < 1):
        raise B4CError('%s: holdout / drop = %d (>= %s), max_len = %d (>= 1)' % (who, holdout, least, max_len))
    return holdout, max_len


def _cloze_rule_args(who, offsets, W, mode, seed, masked_percentage, max_masked, M):
    """the checks cloze_batch and cloze_batch_windows share -> (W, mode, max_masked, M)"""
    mode, max_masked = int(mode), int(max_masked)
    if mode not in (CLOZE_TRAIN, CLOZE_EVAL):
        raise B4CError('%s: mode %d (CLOZE_TRAIN = 0, CLOZE_EVAL = 1)' % (who, mode))
    W = _batch_width(who, W)
    M = (max_masked if mode == CLOZE_TRAIN else 1) if M is None else int(M)
    if not mode <= M <= CLOZE_MAX_LABELS or (mode == CLOZE_TRAIN and not 0 <= max_masked <= M):
        raise B4CError('%s: max_masked = %d, M = %d (0 <= max_masked <= M <= %d; EVAL: M >= 1)' % (who, max_masked, M, CLOZE_MAX_LABELS))
    if mode == CLOZE_TRAIN and not 0.0 <= float(masked_percentage) <= 1.0:
        raise B4CError('%s: masked_percentage %g outside [0, 1]' % (who, masked_percentage))
    if not 0 <= int(seed) < (1 << 64) or offsets.shape[0] - 1 > (1 << 31) - 1:
        raise B4CError('%s: seed %d (0 .. 2^64) / %d sequences (int32 seq_idx)' % (who, seed, offsets.shape[0] - 1))
    return W, mode, max_masked, M


def cloze_batch(items, offsets, seq_idx, W, mode, seed, masked_percentage=0.4, max_masked=10, M=None):
    """-> (items_out int64 [B, W], labels_padded fp32 [B, M], n_masked int32 [B]) (b4c_cloze_batch): row b is sequence
    g = seq_idx[b] of the CSR data set (items int32 [N] label-space indices, offsets int64 [n_seq + 1]) as the model's
    {'asin': items} input -- index + 10, [MASK] = 1 at the masked positions, 0 past the row's length -- with the masked items'
    indices in position order, padded with -1.  mode CLOZE_TRAIN: the last item dropped, n = n_masked(L) positions drawn by the
    keys b4c_rand64(seed, (g << 10) | p) (cloze_choose_host regenerates them); CLOZE_EVAL: the last position masked.
    M: label columns, default max_masked (TRAIN) / 1 (EVAL).  Stream-ordered, nothing is read back: seq_idx is NOT checked
    against n_seq here, and a sequence longer than W is cut at W -- cloze_batches.DeviceCloze checks both on its host copies."""
    items, offsets = _csr_pair('cloze_batch', items, offsets)
    seq_idx = _row_index('cloze_batch', 'seq_idx', seq_idx, 'sequence indices')
    B = seq_idx.shape[0]
    W, mode, max_masked, M = _cloze_rule_args('cloze_batch', offsets, W, mode, seed, masked_percentage, max_masked, M)
    _cuda(items, offsets, seq_idx)
    dev = items.device
    out = torch.empty(B, W, dtype=torch.int64, device=dev)
    lab = torch.empty(B, M, dtype=torch.float32, device=dev)
    nm = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return out, lab, nm
    with _record('cloze_batch', B * (W * 12 + M * 4 + 24)):
        L.check(L.lib().b4c_cloze_batch(_p(items), _p(offsets), _p(seq_idx), B, W, mode, float(masked_percentage), max_masked,
                                        int(seed), _p(out), W, _p(lab), M, M, _p(nm), _st()), 'cloze_batch')
    return out, lab, nm


def cloze_choose_host(seed, g, L, n):
    """-> int32 numpy [n]: the positions of [0, L) that cloze_batch masks in TRAIN mode for sequence g, ascending
    (b4c_cloze_choose: the kernel's rule evaluated on the host, no device work)."""
    import numpy as np
    from . import _lib              # (the argument L, the header's name, hides this module's alias)
    pos = np.empty(max(int(n), 0), dtype=np.int32)
    _lib.check(_lib.lib().b4c_cloze_choose(int(seed) & 0xFFFFFFFFFFFFFFFF, int(g), int(L), int(n), pos.ctypes.data), 'cloze_choose')
    return pos


CLOZE_LAST_ONE = 1 << 24        # last_thr of a last-item rate of 1 (b4c_cloze_batch_windows)


def cloze_last_thr(rate):
    """the integer threshold of a last-item rate in [0, 1]: round(rate * 2^24)"""
    if not 0.0 <= float(rate) <= 1.0:
        raise B4CError('cloze_last_thr: rate %g outside [0, 1]' % rate)
    return int(round(float(rate) * CLOZE_LAST_ONE))


def cloze_batch_windows(items, offsets, win_seq, win_start, win_len, row_win, W, mode, seed, masked_percentage=0.4, max_masked=10, M=None,
                        last_thr=0):
    """-> (items_out int64 [B, W], labels_padded fp32 [B, M], n_masked int32 [B]) (b4c_cloze_batch_windows): row b is window
    w = row_win[b] of the device table (win_seq, win_start, win_len: int32 [n_win]) -- the win_len[w] items of sequence win_seq[w]
    from win_start[w] on -- in cloze_batch's layout.  row_win None: row b is window b; a negative entry: an empty row.
    mode CLOZE_TRAIN: the positions drawn with the window's own seed, or only the last one in a row the last-only draw picks
    (last_thr = cloze_last_thr(rate), 0 .. 2^24; cloze_choose_window_host regenerates both); CLOZE_EVAL: the last position.
    A whole-sequence window (g, 0, n_g - 1) with last_thr = 0 is cloze_batch's TRAIN row.  Stream-ordered, nothing is read back:
    row_win is NOT checked against n_win nor a window against its sequence, and win_len is cut at W."""
    items, offsets = _csr_pair('cloze_batch_windows', items, offsets)
    win_seq, win_start, win_len = _window_table('cloze_batch_windows', win_seq, win_start, win_len)
    row_win = _row_index('cloze_batch_windows', 'row_win', row_win, 'window indices', optional=True)
    B = win_seq.shape[0] if row_win is None else row_win.shape[0]
    W, mode, max_masked, M = _cloze_rule_args('cloze_batch_windows', offsets, W, mode, seed, masked_percentage, max_masked, M)
    last_thr = int(last_thr)
    if mode == CLOZE_TRAIN and (not 0 <= last_thr <= CLOZE_LAST_ONE or (last_thr > 0 and M < 1)):
        raise B4CError('cloze_batch_windows: last_thr = %d (0 .. 2^24 = %d; > 0 needs M >= 1), M = %d' % (last_thr, CLOZE_LAST_ONE, M))
    if mode == CLOZE_EVAL:
        last_thr = 0
    _cuda(items, offsets, win_seq, win_start, win_len, row_win)
    dev = items.device
    out = torch.empty(B, W, dtype=torch.int64, device=dev)
    lab = torch.empty(B, M, dtype=torch.float32, device=dev)
    nm = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return out, lab, nm
    with _record('cloze_batch', B * (W * 12 + M * 4 + 40)):
        L.check(L.lib().b4c_cloze_batch_windows(_p(items), _p(offsets), _p(win_seq), _p(win_start), _p(win_len), _p(row_win), B, W, mode,
                                                float(masked_percentage), max_masked, int(seed), last_thr, _p(out), W, _p(lab), M, M,
                                                _p(nm), _st()), 'cloze_batch_windows')
    return out, lab, nm


def cloze_choose_window_host(seed, g, a, L, masked_percentage=0.4, max_masked=10, last_thr=0):
    """-> int32 numpy [n]: the positions of [0, L) that cloze_batch_windows masks in TRAIN mode for the window of L items at
    start a of sequence g, ascending (b4c_cloze_choose_window: the kernel's rule evaluated on the host, no device work)."""
    import ctypes
    import numpy as np
    from . import _lib              # (the argument L, the header's name, hides this module's alias)
    if not 0 <= int(max_masked) <= CLOZE_MAX_LABELS or not 0 <= int(last_thr) <= CLOZE_LAST_ONE:
        raise B4CError('cloze_choose_window: max_masked = %d (0 .. %d), last_thr = %d (0 .. 2^24)' % (max_masked, CLOZE_MAX_LABELS, last_thr))
    pos = np.empty(max(int(max_masked), 1), dtype=np.int32)
    n = ctypes.c_int32(0)
    _lib.check(_lib.lib().b4c_cloze_choose_window(int(seed) & 0xFFFFFFFFFFFFFFFF, int(g), int(a), int(L), float(masked_percentage),
                                                  int(max_masked), int(last_thr), pos.ctypes.data, ctypes.addressof(n)), 'cloze_choose_window')
    return pos[:n.value].copy()


def cloze_history(items, offsets, seq_idx, E, drop=1):
    """-> int32 [B, E] device tensor (b4c_cloze_history): row b holds the items of sequence seq_idx[b] in front of its target --
    item n_g - drop --, the most recent E when there are more, then -1.  A negative seq_idx: all -1.  The `exclude=` of
    predict_topk, of the ranking metrics and of cloze.sample_candidates takes it (through ops.exclusions).  Stream-ordered,
    nothing is read back: seq_idx is NOT checked against n_seq."""
    items, offsets = _csr_pair('cloze_history', items, offsets)
    seq_idx = _row_index('cloze_history', 'seq_idx', seq_idx, 'sequence indices')
    E, drop = int(E), int(drop)
    if not 1 <= E <= L.MAX_EXCL or drop < 1:
        raise B4CError('cloze_history: E = %d (1 .. %d = B4C_MAX_EXCL), drop = %d (>= 1)' % (E, L.MAX_EXCL, drop))
    _cuda(items, offsets, seq_idx)
    B = seq_idx.shape[0]
    out = torch.empty(B, E, dtype=torch.int32, device=items.device)
    if B:
        with _record('cloze_history', B * (E * 8 + 20)):
            L.check(L.lib().b4c_cloze_history(_p(items), _p(offsets), _p(seq_idx), B, drop, E, _p(out), E, _st()), 'cloze_history')
    return out


NEXT_TRAIN, NEXT_EVAL = L.NEXT_TRAIN, L.NEXT_EVAL            # modes of next_item_batch (include/b4c.h)
NEXT_EXCLUDE = {None: L.NEXT_EXCL_NONE, 'history': L.NEXT_EXCL_HISTORY}


def _next_item_args(who, W, mode, holdout, max_len, V, num_negatives, seed, exclude):
    """the checks next_item_batch and next_item_row_host share -> (W, mode, holdout, max_len, V, N, excl code)"""
    mode, V, N = int(mode), int(V), int(num_negatives)
    if mode not in (NEXT_TRAIN, NEXT_EVAL):
        raise B4CError('%s: mode %d (NEXT_TRAIN = 0, NEXT_EVAL = 1)' % (who, mode))
    W = _batch_width(who, W)
    holdout, max_len = _holdout_args(who, holdout, max_len, 1 if mode == NEXT_EVAL else 0, mode == NEXT_EVAL)
    if V <= 0 or not 0 <= N < L.MAX_CAND:
        raise B4CError('%s: V = %d, num_negatives = %d (0 .. %d)' % (who, V, N, L.MAX_CAND - 1))
    if exclude not in NEXT_EXCLUDE:
        raise B4CError("%s: exclude %r ('history' or None)" % (who, exclude))
    if not 0 <= int(seed) < (1 << 64):
        raise B4CError('%s: seed %d (0 .. 2^64)' % (who, seed))
    return W, mode, holdout, max_len, V, N, NEXT_EXCLUDE[exclude]


def next_item_batch(items, offsets, win_seq, win_start, win_len, row_win, row_off, W, mode, n_targets, V, holdout=1, max_len=None,
                    num_negatives=0, seed=0, exclude='history', item_cdf=None, rows=None):
    """-> (items_out int64 [B, W], flat_idx int32 [rows], labels int32 [rows], cand int32 [rows, 1 + N] or None, short int32 [1])
    (b4c_next_item_batch, include/b4c.h): the next-item batch of the rows row_win -- NEXT_TRAIN: windows of the device
    table (win_seq, win_start, win_len), every input position's target the item after it; NEXT_EVAL: sequences, one target each
    (item n_g - holdout) behind the most recent max_len inputs; a negative entry: an empty row.  No [MASK] anywhere.
    row_off int32 [B + 1]: the exclusive prefix sum of the rows' target counts, on the device; n_targets = row_off[B] as the HOST
    knows it (nothing is read back); rows (default n_targets) compact rows come back, those past n_targets all -1.
    num_negatives N > 0: cand[r] = [label, N negatives], each list what ops.sample_candidates draws for that one target with
    row_base = the target token's CSR index, excluding ('history') the sequence's items in front of the held-out ones.
    Stream-ordered: row_win and the table are NOT checked against the data set."""
    items, offsets = _csr_pair('next_item_batch', items, offsets)
    W, mode, holdout, max_len, V, N, excl = _next_item_args('next_item_batch', W, mode, holdout, max_len, V, num_negatives, seed, exclude)
    win_seq, win_start, win_len = _window_table('next_item_batch', win_seq, win_start, win_len, read=mode == NEXT_TRAIN)
    row_win = _row_index('next_item_batch', 'row_win', row_win, 'window (TRAIN) or sequence (EVAL) indices')
    B = row_win.shape[0]
    if not isinstance(row_off, torch.Tensor) or row_off.dtype != torch.int32 or row_off.dim() != 1 or row_off.shape[0] != B + 1:
        raise B4CError('next_item_batch: row_off must be an int32 [B + 1] = [%d] tensor' % (B + 1))
    R = int(n_targets)
    rows = R if rows is None else int(rows)
    if R < 0 or rows < R:
        raise ValueError('next_item_batch: rows = %d for %d targets' % (rows, R))
    if B * (W + 3) >= 1 << 31:
        raise B4CError('next_item_batch: B (W + 3) = %d does not fit the int32 flat_idx' % (B * (W + 3)))
    if item_cdf is not None:
        if not isinstance(item_cdf, torch.Tensor) or item_cdf.dtype != torch.int64 or item_cdf.dim() != 1 or item_cdf.shape[0] != V:
            raise B4CError('next_item_batch: item_cdf must be an int64 [V] = [%d] prefix sum of item counts' % V)
        item_cdf = item_cdf.contiguous()
    _cuda(items, offsets, win_seq, win_start, win_len, row_win, row_off, item_cdf)
    row_off = row_off.contiguous()
    dev = items.device
    out = torch.empty(B, W, dtype=torch.int64, device=dev)
    alloc = max(rows, 1)            # (a batch without a target still hands the entry point real pointers)
    flat_buf = torch.empty(alloc, dtype=torch.int32, device=dev)
    lab_buf = torch.empty(alloc, dtype=torch.int32, device=dev)
    cand_buf = torch.empty(alloc, N + 1, dtype=torch.int32, device=dev) if N > 0 else None
    flat, lab, cand = flat_buf[:rows], lab_buf[:rows], None if cand_buf is None else cand_buf[:rows]
    short = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0:
        flat.fill_(-1)
        lab.fill_(-1)
        if cand is not None:
            cand.fill_(-1)
        return out, flat, lab, cand, short
    with _record('next_item_batch', B * (W * 12 + 40) + rows * (8 + (N + 1) * 4 if N else 8)):
        L.check(L.lib().b4c_next_item_batch(_p(items), _p(offsets), _p(win_seq), _p(win_start), _p(win_len), _p(row_win), _p(row_off), B, W,
                                            mode, holdout, max_len, V, N, int(seed), excl, _p(item_cdf), _p(out), W, _p(flat_buf),
                                            _p(lab_buf), _p(cand_buf), N + 1, rows, _p(short) if N > 0 else None, _st()), 'next_item_batch')
    return out, flat, lab, cand, short


def next_item_row_host(seq, seq_off, W, mode, V, a=0, L=0, holdout=1, max_len=None, num_negatives=0, seed=0, exclude='history',
                       item_cdf=None):
    """-> dict(inputs int64 [W], labels int32 [n], pos int32 [n], candidates int32 [n, 1 + N] or None, n_in, short) in numpy
    (b4c_next_item_row: next_item_batch's rule for ONE row evaluated on the host, no device work).  seq: the items of sequence g,
    seq_off = offsets[g]; (a, L): the window (TRAIN).  item_cdf: a host int64 [V] array."""
    import ctypes
    import numpy as np
    from . import _lib              # (the argument L, the header's name, hides this module's alias)
    W, mode, holdout, max_len, V, N, excl = _next_item_args('next_item_row', W, mode, holdout, max_len, V, num_negatives, seed, exclude)
    seq = np.ascontiguousarray(seq, dtype=np.int32).reshape(-1)
    if int(a) < 0 or int(L) < 0 or int(seq_off) < 0:
        raise B4CError('next_item_row: window (a = %d, L = %d), seq_off = %d' % (a, L, seq_off))
    cdf = None
    if item_cdf is not None:
        cdf = np.ascontiguousarray(item_cdf, dtype=np.int64).reshape(-1)
        if cdf.shape[0] != V:
            raise B4CError('next_item_row: item_cdf must be an int64 [V] = [%d] prefix sum of item counts' % V)
    inputs = np.empty(W, dtype=np.int64)
    lab, pos = np.empty(W, dtype=np.int32), np.empty(W, dtype=np.int32)
    cand = np.empty((W, N + 1), dtype=np.int32) if N > 0 else None
    counts = (ctypes.c_int32 * 3)()
    _lib.check(_lib.lib().b4c_next_item_row(seq.ctypes.data if len(seq) else None, len(seq), int(seq_off), int(a), int(L), W, mode, holdout,
                                            max_len, V, N, int(seed), excl, None if cdf is None else cdf.ctypes.data, inputs.ctypes.data,
                                            lab.ctypes.data, pos.ctypes.data, None if cand is None else cand.ctypes.data, N + 1,
                                            ctypes.addressof(counts)), 'next_item_row')
    n = int(counts[1])
    return {'inputs': inputs, 'labels': lab[:n].copy(), 'pos': pos[:n].copy(), 'candidates': None if cand is None else cand[:n].copy(),
            'n_in': int(counts[0]), 'short': int(counts[2])}


# ---- side features beside the items of a device-built batch (include/b4c.h) ----
FEAT_EVENT, FEAT_ITEM = L.FEAT_EVENT, L.FEAT_ITEM                  # where a feature's value comes from: the token / the item
FEAT_MASKED, FEAT_KEPT = L.FEAT_MASKED, L.FEAT_KEPT                # what a [MASK] of the item row does to the feature
FEAT_CLOZE, FEAT_NEXT_TRAIN, FEAT_NEXT_EVAL = L.FEAT_CLOZE, L.FEAT_NEXT_TRAIN, L.FEAT_NEXT_EVAL      # the row geometry
FEAT_KINDS = {'event': FEAT_EVENT, 'item': FEAT_ITEM}
FEAT_ON_MASK = {'mask': FEAT_MASKED, 'keep': FEAT_KEPT}
FEAT_LAYOUTS = (FEAT_CLOZE, FEAT_NEXT_TRAIN, FEAT_NEXT_EVAL)


def _batch_features_args(who, W, layout, holdout, max_len, per, on_mask):
    """the checks batch_features and batch_features_row_host share -> (W, layout, holdout, max_len, kind code, on_mask code)"""
    layout = int(layout)
    if layout not in FEAT_LAYOUTS:
        raise B4CError('%s: layout %d (FEAT_CLOZE = 0, FEAT_NEXT_TRAIN = 1, FEAT_NEXT_EVAL = 2)' % (who, layout))
    W = _batch_width(who, W)
    holdout, max_len = _holdout_args(who, holdout, max_len, None if layout == FEAT_CLOZE else 1, layout != FEAT_CLOZE)
    if per not in FEAT_KINDS:
        raise B4CError("%s: per %r ('event' or 'item')" % (who, per))
    if on_mask not in FEAT_ON_MASK:
        raise B4CError("%s: on_mask %r ('mask' or 'keep')" % (who, on_mask))
    return W, layout, holdout, max_len, FEAT_KINDS[per], FEAT_ON_MASK[on_mask]


def batch_features(items, offsets, win_seq, win_start, win_len, row_win, W, layout, items_in, sources, holdout=1, max_len=None):
    """-> [out_f int64 [B, W] for every source] (b4c_batch_features, include/b4c.h): the side features of the batch
    rows whose item row items_in int64 [B, >= W] has just been built -- layout FEAT_CLOZE: by cloze_batch_windows from the windows
    row_win of the device table (win_seq, win_start, win_len); FEAT_NEXT_TRAIN / FEAT_NEXT_EVAL: by next_item_batch in that mode
    with the same holdout / max_len (EVAL: row_win names sequences, the table is not read).  row_win None: row b is window b.
    sources: up to B4C_MAX_FEATURES triples (src int32 device tensor, per, on_mask) -- per 'event': src [n_items] is aligned with
    `items`; 'item': src [V] is a table over the items; on_mask 'mask': [MASK] where the item row has it, 'keep': the value.
    Ids are value + 10, 0 past the row.  One launch for all sources, stream-ordered, nothing is read back: neither the rows nor
    the values are range-checked (cloze_batches.DeviceCloze checks its features on the host, once)."""
    items, offsets = _csr_pair('batch_features', items, offsets)
    sources = list(sources)
    if not 1 <= len(sources) <= L.MAX_FEATURES:
        raise B4CError('batch_features: %d sources (1 .. %d = B4C_MAX_FEATURES)' % (len(sources), L.MAX_FEATURES))
    codes, V = [], 0
    for f, source in enumerate(sources):
        if len(source) != 3:
            raise B4CError('batch_features: source %d must be (src, per, on_mask)' % f)
        src, per, on_mask = source
        W, layout, holdout_c, max_len_c, kind, keep = _batch_features_args('batch_features', W, layout, holdout, max_len, per, on_mask)
        if not isinstance(src, torch.Tensor) or src.dim() != 1 or src.dtype != torch.int32:
            raise B4CError('batch_features: src of source %d must be an int32 one-dimensional tensor' % f)
        if kind == FEAT_EVENT and src.shape[0] != items.shape[0]:
            raise B4CError("batch_features: source %d is per 'event': %d values for %d tokens" % (f, src.shape[0], items.shape[0]))
        if kind == FEAT_ITEM:
            if src.shape[0] < 1 or (V and src.shape[0] != V):
                raise B4CError("batch_features: source %d is per 'item': a table of %d entries (another has %d)" % (f, src.shape[0], V))
            V = int(src.shape[0])
        codes.append((kind, keep))
    win_seq, win_start, win_len = _window_table('batch_features', win_seq, win_start, win_len, read=layout != FEAT_NEXT_EVAL)
    if not isinstance(items_in, torch.Tensor) or items_in.dim() != 2 or items_in.dtype != torch.int64 or items_in.shape[1] < W:
        raise B4CError('batch_features: items_in must be the int64 [B, >= W = %d] item rows' % W)
    B = items_in.shape[0]
    row_win = _row_index('batch_features', 'row_win', row_win, 'window (EVAL: sequence) indices', B=B, optional=True)
    srcs = [s[0] for s in sources]
    _cuda(items, offsets, win_seq, win_start, win_len, row_win, items_in, *srcs)
    if B and items_in.stride(1) != 1:
        items_in = items_in.contiguous()
    srcs = [s.contiguous() for s in srcs]
    outs = [torch.empty(B, W, dtype=torch.int64, device=items.device) for _ in srcs]
    if B == 0:
        return outs
    n = len(srcs)
    src_arr = (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs])
    out_arr = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    kind_arr = (ctypes.c_int * n)(*[c[0] for c in codes])
    keep_arr = (ctypes.c_int * n)(*[c[1] for c in codes])
    with _record('batch_features', B * (W * 8 * (n + 1) + W * 4 * (n + 1) + 40)):
        L.check(L.lib().b4c_batch_features(_p(items), _p(offsets), _p(win_seq), _p(win_start), _p(win_len), _p(row_win), B, W, layout,
                                           holdout_c, max_len_c, V, _p(items_in), int(items_in.stride(0)), n, src_arr, kind_arr, keep_arr,
                                           out_arr, W, _st()), 'batch_features')
    return outs


def batch_features_row_host(seq, seq_off, W, layout, src, per, on_mask, items_in, a=0, L=0, holdout=1, max_len=None):
    """-> (out int64 numpy [W], first, n) (b4c_batch_features_row: batch_features' rule for ONE row and ONE source evaluated on the
    host, no device work).  seq: the items of sequence g, seq_off = offsets[g]; (a, L): the window (ignored for FEAT_NEXT_EVAL);
    src: the WHOLE source array (per 'event': one value per token of the data set; 'item': the table); items_in: the item row."""
    import numpy as np
    from . import _lib              # (the argument L, the header's name, hides this module's alias)
    W, layout, holdout, max_len, kind, keep = _batch_features_args('batch_features_row', W, layout, holdout, max_len, per, on_mask)
    seq = np.ascontiguousarray(seq, dtype=np.int32).reshape(-1)
    src = np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
    items_in = np.ascontiguousarray(items_in, dtype=np.int64).reshape(-1)
    if int(a) < 0 or int(L) < 0 or int(seq_off) < 0:
        raise B4CError('batch_features_row: window (a = %d, L = %d), seq_off = %d' % (a, L, seq_off))
    if items_in.shape[0] < W:
        raise B4CError('batch_features_row: items_in holds %d columns, W = %d' % (items_in.shape[0], W))
    if kind == FEAT_EVENT and src.shape[0] < int(seq_off) + len(seq):
        raise B4CError("batch_features_row: per 'event': %d values, the sequence ends at token %d" % (src.shape[0], int(seq_off) + len(seq)))
    if len(src) < 1:
        raise B4CError('batch_features_row: an empty source')
    out = np.empty(W, dtype=np.int64)
    geom = (ctypes.c_int32 * 2)()
    _lib.check(_lib.lib().b4c_batch_features_row(seq.ctypes.data if len(seq) else None, len(seq), int(seq_off), int(a), int(L), W, layout,
                                                 holdout, max_len, len(src) if kind == FEAT_ITEM else 0, src.ctypes.data, kind, keep,
                                                 items_in.ctypes.data, out.ctypes.data, ctypes.addressof(geom)), 'batch_features_row')
    return out, int(geom[0]), int(geom[1])


# ---- contrastive views of a device-built batch (include/b4c.h): crop, mask, reorder, the same-target row ----
AUG_OPS = {'crop': L.AUG_CROP, 'mask': L.AUG_MASK, 'reorder': L.AUG_REORDER, 'same_target': L.AUG_SAME_TARGET}      # name -> op bit
AUG_LAYOUTS = (FEAT_CLOZE, FEAT_NEXT_TRAIN)


def _augment_args(who, W, layout, holdout, max_len, n_views, view_ops, seed, crop_ratio, mask_ratio, reorder_ratio):
    """the checks augment_views and augment_row_host share -> (W, layout, holdout, max_len, n_views, ops_mask, the three ratios)"""
    layout, n_views = int(layout), int(n_views)
    if layout not in AUG_LAYOUTS:
        raise B4CError('%s: layout %d (FEAT_CLOZE = 0 or FEAT_NEXT_TRAIN = 1; views of evaluation rows are not built)' % (who, layout))
    W = _batch_width(who, W)
    holdout, max_len = _holdout_args(who, holdout, max_len, None if layout == FEAT_CLOZE else 0, False)
    if not 1 <= n_views <= L.AUG_MAX_VIEWS:
        raise B4CError('%s: n_views = %d (1 .. %d)' % (who, n_views, L.AUG_MAX_VIEWS))
    view_ops = (view_ops,) if isinstance(view_ops, str) else tuple(view_ops)
    if not view_ops or any(o not in AUG_OPS for o in view_ops):
        raise B4CError('%s: ops %r (one or more of %s)' % (who, view_ops, ', '.join(repr(o) for o in AUG_OPS)))
    mask = 0
    for o in view_ops:
        mask |= AUG_OPS[o]
    if mask & L.AUG_SAME_TARGET and layout != FEAT_NEXT_TRAIN:
        raise B4CError("%s: 'same_target' needs the next-item layout (a Cloze row has no target)" % who)
    crop_ratio, mask_ratio, reorder_ratio = float(crop_ratio), float(mask_ratio), float(reorder_ratio)
    if not 0.0 < crop_ratio <= 1.0 or not 0.0 <= mask_ratio <= 1.0 or not 0.0 <= reorder_ratio <= 1.0:
        raise B4CError('%s: crop_ratio = %g (0 < . <= 1), mask_ratio = %g, reorder_ratio = %g (0 <= . <= 1)'
                       % (who, crop_ratio, mask_ratio, reorder_ratio))
    if not 0 <= int(seed) < (1 << 64):
        raise B4CError('%s: seed %d (0 .. 2^64)' % (who, seed))
    return W, layout, holdout, max_len, n_views, mask, crop_ratio, mask_ratio, reorder_ratio


def augment_views(items, offsets, win_seq, win_start, win_len, row_win, W, layout, view_ops, seed, n_views=2, holdout=1, max_len=None,
                  crop_ratio=0.6, mask_ratio=0.3, reorder_ratio=0.6, target_index=None, V=0):
    """-> (items_out int64 [n_views, B, W], src_tok int64 [n_views, B, W], n_items, op, target int32 [n_views, B], self_count int32
    [1]) (b4c_augment_views, include/b4c.h): n_views contrastive views of the batch rows row_win (windows of the device table)
    whose item rows cloze_batch_windows (layout FEAT_CLOZE) or next_item_batch in TRAIN mode (FEAT_NEXT_TRAIN, the same holdout)
    built.  Per (row, view) one of view_ops is drawn -- 'crop': a contiguous slice of crop_ratio of the row; 'mask': mask_ratio of
    its positions become [MASK]; 'reorder': a span of reorder_ratio of the row is shuffled; 'same_target' (next-item only): the
    items in front of another occurrence of the row's target item, of any sequence, the most recent min(W, max_len) of them -- the
    row itself where there is none (self_count counts those).  target_index = (tgt_first int64 [V + 1], tgt_tok int64 [n],
    tgt_seq int32 [n]) on the device, with V: 'same_target' needs it.  src_tok: the CSR index of every output position's token, -1
    at pad; op: the drawn op's bit (ops.AUG_OPS); target: the row's target item (next-item), -1 for Cloze rows.  A row is a pure
    function of (seed, view, window).  Stream-ordered, nothing is read back; rows and index are not checked against the data set."""
    who = 'augment_views'
    items, offsets = _csr_pair(who, items, offsets)
    W, layout, holdout, max_len, n_views, mask, crop_ratio, mask_ratio, reorder_ratio = _augment_args(
        who, W, layout, holdout, max_len, n_views, view_ops, seed, crop_ratio, mask_ratio, reorder_ratio)
    win_seq, win_start, win_len = _window_table(who, win_seq, win_start, win_len)
    row_win = _row_index(who, 'row_win', row_win, 'window indices')
    B = row_win.shape[0]
    idx = (None, None, None)
    if mask & L.AUG_SAME_TARGET:
        V = int(V)
        ok = target_index is not None and len(target_index) == 3 and all(isinstance(t, torch.Tensor) and t.dim() == 1 for t in target_index)
        if not ok or V < 1 or target_index[0].dtype != torch.int64 or target_index[0].shape[0] != V + 1 or target_index[1].dtype != torch.int64 \
                or target_index[2].dtype != torch.int32 or target_index[1].shape != target_index[2].shape:
            raise B4CError("%s: 'same_target' needs target_index = (tgt_first int64 [V + 1], tgt_tok int64 [n], tgt_seq int32 [n]) and V > 0"
                           % who)
        idx = tuple(t.contiguous() for t in target_index)
    _cuda(items, offsets, win_seq, win_start, win_len, row_win, *idx)
    dev = items.device
    out = torch.empty(n_views, B, W, dtype=torch.int64, device=dev)
    tok = torch.empty(n_views, B, W, dtype=torch.int64, device=dev)
    n_out = torch.empty(n_views, B, dtype=torch.int32, device=dev)
    op = torch.empty(n_views, B, dtype=torch.int32, device=dev)
    target = torch.empty(n_views, B, dtype=torch.int32, device=dev)
    self_count = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0:
        return out, tok, n_out, op, target, self_count
    with _record(who, n_views * B * (W * 20 + 40)):
        L.check(L.lib().b4c_augment_views(_p(items), _p(offsets), _p(win_seq), _p(win_start), _p(win_len), _p(row_win), B, W, layout, holdout,
                                          max_len, n_views, mask, crop_ratio, mask_ratio, reorder_ratio, int(seed), _p(idx[0]), _p(idx[1]),
                                          _p(idx[2]), V if mask & L.AUG_SAME_TARGET else 0, _p(out), W, _p(tok), W, _p(n_out), _p(op),
                                          _p(target), _p(self_count), _st()), who)
    return out, tok, n_out, op, target, self_count


def augment_row_host(items, offsets, g, W, layout, view_ops, seed, view=0, a=0, L=0, holdout=1, max_len=None, crop_ratio=0.6,
                     mask_ratio=0.3, reorder_ratio=0.6, target_index=None, V=0):
    """-> dict(items int64 [W], src_tok int64 [W], n_items, op, target, self) in numpy and ints (b4c_augment_row: augment_views' rule
    for ONE row and ONE view evaluated on the host, no device work).  items / offsets: the whole CSR pair as host arrays; (g, a, L):
    the window, g < 0: an empty row; target_index: host arrays."""
    import numpy as np
    from . import _lib              # (the argument L, the header's name, hides this module's alias)
    who = 'augment_row'
    W, layout, holdout, max_len, _, mask, crop_ratio, mask_ratio, reorder_ratio = _augment_args(
        who, W, layout, holdout, max_len, 1, view_ops, seed, crop_ratio, mask_ratio, reorder_ratio)
    items = np.ascontiguousarray(items, dtype=np.int32).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    idx = [None, None, None]
    if mask & _lib.AUG_SAME_TARGET:
        if target_index is None or len(target_index) != 3 or int(V) < 1:
            raise B4CError("%s: 'same_target' needs target_index = (tgt_first, tgt_tok, tgt_seq) and V > 0" % who)
        idx = [np.ascontiguousarray(t, dtype=dt).reshape(-1) for t, dt in zip(target_index, (np.int64, np.int64, np.int32))]
        if len(idx[0]) != int(V) + 1 or len(idx[1]) != len(idx[2]):
            raise B4CError('%s: tgt_first holds %d entries for V = %d; tgt_tok %d, tgt_seq %d' % (who, len(idx[0]), V, len(idx[1]), len(idx[2])))
    out, tok = np.empty(W, dtype=np.int64), np.empty(W, dtype=np.int64)
    head = (ctypes.c_int32 * 4)()
    ptr = lambda x: None if x is None or not len(x) else x.ctypes.data
    _lib.check(_lib.lib().b4c_augment_row(items.ctypes.data, offsets.ctypes.data, len(offsets) - 1, int(g), int(a), int(L), W, layout, holdout,
                                          max_len, int(view), mask, crop_ratio, mask_ratio, reorder_ratio, int(seed), ptr(idx[0]), ptr(idx[1]),
                                          ptr(idx[2]), int(V) if mask & _lib.AUG_SAME_TARGET else 0, out.ctypes.data, tok.ctypes.data,
                                          ctypes.addressof(head)), who)
    return {'items': out, 'src_tok': tok, 'n_items': int(head[0]), 'op': int(head[1]), 'target': int(head[2]), 'self': int(head[3])}


def adam_step_(p, g, m, v, lr_t, beta1, beta2, eps, grad_mul=1.0, coef=None, decay=None, blocks=None):
    """Dense Adam over a flat fp32 range (b4c_adam_step).  coef (device fp32 scalar of grad_clip_coef_): the gradient is scaled by
    grad_mul * coef[0] (b4c_adam_step_clipped).  decay: decoupled weight decay -- the elements of the 64-element blocks flagged in
    `blocks` (uint8, one per block of p) take p <- p - decay * p first (b4c_adamw_step; coef may still be None)."""
    lib, args = L.lib(), (_p(p), _p(g), _p(m), _p(v), p.numel(), lr_t, beta1, beta2, eps, grad_mul)
    with _record('adam', p.numel() * 28 + (blocks.numel() if decay is not None else 0)):
        if decay is not None:
            L.check(lib.b4c_adamw_step(*args, _p(coef), decay, _p(blocks), _st()), 'adamw_step')
        elif coef is not None:
            L.check(lib.b4c_adam_step_clipped(*args, _p(coef), _st()), 'adam_step_clipped')
        else:
            L.check(lib.b4c_adam_step(*args, _st()), 'adam_step')


def adam_rows_(p, g, m, v, stamp, ids, n, row_lo, rows, width, lr_hist, t, beta1, beta2, eps, grad_mul, mode, coef=None, decay_hist=None):
    """b4c_adam_rows over one row-sparse table of the arena (optim.LazyRows): mode 0 = bring rows to step t, 1 = take step t.
    coef (device fp32 scalar): the step's gradient is scaled by grad_mul * coef[0] (b4c_adam_rows_clipped).  decay_hist: the table
    decays, decay_hist[s] beside lr_hist[s] (b4c_adamw_rows; coef may still be None).
    Booked bytes: the rows NAMED (an upper bound of the distinct rows; rec_hints['adam_distinct_rows'] when the host knows it)."""
    if n <= 0:
        return
    nrows = min(n, rec_hints.get('adam_distinct_rows', n)) if ids is not None else n
    lib, args = L.lib(), (_p(p), _p(g), _p(m), _p(v), _p(stamp), _p(ids), n, row_lo, rows, width, _p(lr_hist))
    with _record('adam' if mode == 1 else 'adam_catch_up', nrows * width * (32 if mode == 1 else 24) + (n * 8 if ids is not None else 0)):
        if decay_hist is not None:
            L.check(lib.b4c_adamw_rows(*args, _p(decay_hist), t, beta1, beta2, eps, grad_mul, _p(coef), mode, _st()), 'adamw_rows')
        elif coef is not None:
            L.check(lib.b4c_adam_rows_clipped(*args, t, beta1, beta2, eps, grad_mul, _p(coef), mode, _st()), 'adam_rows_clipped')
        else:
            L.check(lib.b4c_adam_rows(*args, t, beta1, beta2, eps, grad_mul, mode, _st()), 'adam_rows')


def grad_chunks(n):
    """number of chunk partials of an arena of n elements (b4c_grad_sumsq)"""
    return (n + L.GRAD_CHUNK - 1) // L.GRAD_CHUNK


def grad_sumsq_(grad, lo, hi, partial):
    """partial[c] (float64) := sum of squares of every chunk of the fp32 arena `grad` that overlaps [lo, hi) (csrc/gradnorm.hip)"""
    if hi <= lo:
        return
    c = grad_chunks(hi) - lo // L.GRAD_CHUNK
    with _record('grad_norm', c * (L.GRAD_CHUNK * 4 + 8)):
        L.check(L.lib().b4c_grad_sumsq(_p(grad), grad.numel(), lo, hi, _p(partial), _st()), 'grad_sumsq')


def grad_sumsq_rows_(grad, table_lo, rows, width, ids, partial):
    """the same for the chunks that the rows `ids` (int64, contiguous; repeats and out-of-range values as adam_rows_ takes
    them) of the (rows, width) table at grad[table_lo:] overlap.  Booked bytes: every named row's chunks (an upper bound)."""
    n = ids.numel()
    if n <= 0:
        return
    per = (width + L.GRAD_CHUNK - 1) // L.GRAD_CHUNK + 1          # (a row of `width` elements overlaps at most this many chunks)
    with _record('grad_norm', n * (8 + per * (L.GRAD_CHUNK * 4 + 8))):
        L.check(L.lib().b4c_grad_sumsq_rows(_p(grad), grad.numel(), table_lo, rows, width, _p(ids), n, _p(partial), _st()),
                'grad_sumsq_rows')


def grad_clip_coef_(partial, group_sums, clip, grad_mul, total, norm_coef):
    """total (float64 [1], may be None) := fixed tree over `partial`; norm_coef (fp32 [2]) := (sqrt(total) |grad_mul|, clip
    coefficient: exactly 1 when the norm is <= clip, NaN when it is not finite).  All on the device."""
    with _record('grad_norm', partial.numel() * 8 + group_sums.numel() * 16 + 16):
        L.check(L.lib().b4c_grad_clip_coef(_p(partial), partial.numel(), _p(group_sums), group_sums.numel(), clip, grad_mul,
                                           _p(total), _p(norm_coef), _st()), 'grad_clip_coef')


def rand64_host(seed, ctr):
    """Host restatement of b4c_rand64 (csrc/common.h): Threefry-2x32, 12 rounds, key = seed, counter = ctr (uint64 array)."""
    import numpy as np
    M = np.uint64(0xFFFFFFFF)

    def rotl(x, r):
        return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & M

    ctr = np.asarray(ctr, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    k2 = np.uint64(0x1BD11BDA) ^ k0 ^ k1
    x0 = ((ctr & M) + k0) & M
    x1 = ((ctr >> np.uint64(32)) + k1) & M
    inject = [(k1, k2, 1), (k2, k0, 2), (k0, k1, 3)]
    rounds = [(13, 15, 26, 6), (17, 29, 16, 24), (13, 15, 26, 6)]
    for rs, (a0, a1, j) in zip(rounds, inject):
        for r in rs:
            x0 = (x0 + x1) & M
            x1 = rotl(x1, r) ^ x0
        x0 = (x0 + a0) & M
        x1 = (x1 + a1 + np.uint64(j)) & M
    return x0 | (x1 << np.uint64(32))



def mulhi64_host(x, v):
    """Host restatement of the sampler's mulhi64 (csrc/candidates.hip): the high 64 bits of the 128-bit product of uint64 x
    (array) and 0 <= v < 2^64 (an integer, or an array that broadcasts against x), exact (32-bit halves)."""
    import numpy as np
    M = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    x = np.asarray(x, dtype=np.uint64)
    if isinstance(v, np.ndarray):
        v = v.astype(np.uint64)
        vl, vh = v & M, v >> s32
    else:
        v = int(v)
        vl, vh = np.uint64(v & 0xFFFFFFFF), np.uint64(v >> 32)
    xl, xh = x & M, x >> s32
    t = xl * vl
    m1 = xh * vl + (t >> s32)
    m2 = xl * vh + (m1 & M)
    return xh * vh + (m1 >> s32) + (m2 >> s32)

def keep_mask(seed, n, rate):
    """Host regeneration of a dropout keep-mask (tests): element e kept iff b4c_keep(seed, e, rate) --
    counter = e >> 2, one 16-bit uniform per element (csrc/common.h)."""
    import numpy as np
    e = np.arange(n, dtype=np.uint64)
    h = rand64_host(seed, e >> np.uint64(2))
    u16 = (h >> (np.uint64(16) * (e & np.uint64(3)))) & np.uint64(0xFFFF)
    t = np.float32(rate) * np.float32(65536.0)
    thr = int(t)
    if np.float32(thr) < t:
        thr += 1
    return u16 >= np.uint64(thr)


# --------------------------------------------------------------------------------------
# packed compute copies of (fused) dense layers
# --------------------------------------------------------------------------------------
_pack_registry = []      # weak references to every PackedLinear: stale ones are refreshed together, in one launch


class PackedLinear:
    """Compute-dtype copies of one dense layer whose Keras kernels [K, N_i] are fused along N:
    ``wt`` [Np][Kp] (forward operand, K-contiguous) and ``wc`` [Kp][Np] (backward-dX operand),
    ``bias`` fp32 [Np].  Zero-padded to multiples of 8.  When the masters change (optimizer step,
    load_state_dict, .to()) ALL stale layers are re-packed by one b4c_pack_weights_batched launch."""

    def __init__(self, kernels, biases):
        import weakref
        self.kernels, self.biases = list(kernels), list(biases)
        self.K = int(self.kernels[0].shape[0])
        self.Ns = [int(k.shape[1]) for k in self.kernels]
        self.N = sum(self.Ns)
        self.Np = rup8(self.N)
        self._cache = {}
        _pack_registry.append(weakref.ref(self))

    def _key(self):
        return (_weights_epoch,) + tuple(t._version for t in self.kernels + self.biases) + \
            tuple(t.data_ptr() for t in self.kernels + self.biases)

    def _descs(self, ent, Kp):
        out, off = [], 0
        for k, b, n in zip(self.kernels, self.biases, self.Ns):
            kk = k.detach()
            if kk.dtype != torch.float32 or not kk.is_contiguous():
                raise B4CError('dense kernels must be contiguous float32 [in, out]')
            out.append(L.PackDesc(kk.data_ptr(), b.detach().data_ptr(), ent['wt'].data_ptr(),
                                  ent['wc'].data_ptr() if ent['wc'] is not None else None, ent['bias'].data_ptr(),
                                  self.K, n, Kp, self.Np, off, 0))
            off += n
        return out

    def get(self, dtype, Kp, need_wc):
        dev = self.kernels[0].device
        ent = self._cache.get((dtype, Kp, dev))
        if ent is None:
            ent = {'key': None, 'wt': torch.zeros(self.Np, Kp, dtype=dtype, device=dev), 'wc': None,
                   'bias': torch.zeros(self.Np, dtype=torch.float32, device=dev)}
            self._cache[(dtype, Kp, dev)] = ent
        if need_wc and ent['wc'] is None:
            ent['wc'] = torch.zeros(Kp, self.Np, dtype=dtype, device=dev)
            ent['key'] = None
        if ent['key'] != self._key():
            repack_stale(dtype, dev)
        return ent['wt'], ent['wc'], ent['bias']


_desc_cache = {}


def repack_stale(dtype, dev):
    """One launch refreshes every allocated compute copy (this dtype / device) whose masters changed."""
    descs, ents, tiles = [], [], []
    alive = []
    for ref in _pack_registry:
        pk = ref()
        if pk is None:
            continue
        alive.append(ref)
        key = None
        for (dt, Kp, dv), ent in pk._cache.items():
            if dt != dtype or dv != dev:
                continue
            key = key or pk._key()
            if ent['key'] == key:
                continue
            descs += pk._descs(ent, Kp)
            ents.append((ent, key))
            tiles += [((pk.K + 63) // 64) * ((n + 63) // 64) for n in pk.Ns]       # 64 x 64 tiles (csrc/rowops.hip)
    _pack_registry[:] = alive
    if not descs:
        return
    # The launch is a (largest tile count) x (descriptors) grid whose surplus workgroups exit at once; one vocabulary
    # projection (1,564 tiles of 64 x 64 at C2) beside thirty encoder matrices (4 tiles each) would make that 50,000 workgroups
    # for 1,900 tiles of work.  Descriptors are ordered by size and launched in groups of similar size (a factor of 8).
    order = sorted(range(len(descs)), key=lambda i: tiles[i])
    descs = [descs[i] for i in order]
    tiles = [tiles[i] for i in order]
    sig = tuple((d.src, d.wt, d.wc, d.bias_src) for d in descs)
    cached = _desc_cache.get((dtype, dev))
    if cached is None or cached[0] != sig:
        arr = (L.PackDesc * len(descs))(*descs)
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        cached = (sig, host.to(dev))
        _desc_cache[(dtype, dev)] = cached
    esz = ctypes.sizeof(L.PackDesc)
    with torch.no_grad():
        i0 = 0
        while i0 < len(descs):
            i1 = i0 + 1
            while i1 < len(descs) and tiles[i1] <= 8 * max(tiles[i0], 1):
                i1 += 1
            L.check(L.lib().b4c_pack_weights_batched(cached[1].data_ptr() + i0 * esz, i1 - i0, max(tiles[i1 - 1], 1),
                                                     dt_code(dtype), _st()), 'pack_weights_batched')
            i0 = i1
    for ent, key in ents:
        ent['key'] = key


def _as2d(x):
    return x.reshape(-1, x.shape[-1])


# --------------------------------------------------------------------------------------
# autograd blocks
# --------------------------------------------------------------------------------------
def _embed_stage_fwd(ctx, pe, n, packed, args):
    """What the two input stages do in front of their forward kernel.  args = (*ids, *tables), the LAST 2 n inputs of apply
    -> (dense_ids, ids, tables): ids are the ones the tables' backward works on (packed layout: the packed ids, B = 1, S = T rows)."""
    ids, tables = list(args[:n]), list(args[n:])
    dense_ids = ids
    if packed is not None:
        # one gather per feature
        pk_ids = []
        for i in ids:
            flat = i.reshape(-1)
            if flat.dtype != torch.int64 or not flat.is_contiguous():
                flat = flat.to(torch.int64).contiguous()
            o = torch.empty(1, packed.T, dtype=torch.int64, device=flat.device)
            L.check(L.lib().b4c_gather_i64(_p(flat), _p(packed.tok_src), _p(o), packed.T, _st()), 'gather_i64')
            pk_ids.append(o)
        ids = pk_ids
    # a table under a row-lazy optimizer (optim.LazyRows): the rows about to be read are brought up to date first (a backward
    # that gathers again reads the same, caught-up rows)
    first_table = len(ctx.needs_input_grad) - n
    for j, (t, i) in enumerate(zip(tables, ids)):
        lz = getattr(t, '_b4c_lazy', None)
        if lz is not None:
            lz.catch_up(i, note=ctx.needs_input_grad[first_table + j])
    ctx.pe = pe
    if ctx.needs_input_grad[0]:        # a learned positional table: what its gradient kernel needs
        if packed is not None and packed.packed_of is None:
            raise B4CError('learned positions in the packed layout need Packed.packed_of (the row of every dense position)')
        ctx.seqs = (dense_ids[0].shape[0], dense_ids[0].shape[1], packed.packed_of if packed is not None else None)
    return dense_ids, ids, tables


def _embed_stage_bwd(ctx, ids, tables, g, rate, seed, lead=()):
    """The gradients both input stages end with: g [B, S, d] (packed layout [1, T, d]) is the gradient behind scale * rows + PE,
    (rate, seed) the dropout still to be applied to it.  Adds the learned positional table's and the tables' gradients into their
    sinks and announces them -> autograd's return values; `lead`: the gradients of the inputs right behind pe."""
    dpe = None
    if ctx.needs_input_grad[0]:
        B, S, row_of = ctx.seqs
        # dense layout: sequence b owns rows b*S .. (b+1)*S, pad rows included (the forward adds P there too); packed: the row
        # of a dense position is packed_of's (a Cloze batch pads BEFORE its closing [SEP]: positions are not 0 .. len-1)
        cu = dense_cu(B, S, g.device) if row_of is None else None
        pactx, (psink,) = grad_sinks(ctx.pe)
        pos_table_bwd(g, cu, B, S, rate, seed, psink, row_of=row_of)
        _ready(ctx.pe)
        dpe = None if pactx is not None else psink
    actx, sinks = grad_sinks(*tables)
    embed_concat_pe_bwd(ids, tables, g, ctx.scale, rate, seed, into=sinks)
    _ready(*tables)
    lead = (dpe,) + tuple(lead)
    return sink_returns(ctx, lead + (None,) * (len(ctx.needs_input_grad) - len(tables) - len(lead)), actx, sinks)


class EmbedFn(torch.autograd.Function):
    """R6: gather + concat + *sqrt(d) + PE (+ input dropout).  apply(pe, scale, rate, seed, dtype, packed, combine, n, *ids, *tables);
    packed (Packed or None): the packed layout, output (1, T, d); combine 'concat' or 'sum' (the features' rows are added).
    pe is differentiable when it is a parameter (learned positions): its gradient is b4c_pos_table_bwd's."""

    @staticmethod
    def forward(ctx, pe, scale, rate, seed, dtype, packed, combine, n, *args):
        dense_ids, ids, tables = _embed_stage_fwd(ctx, pe, n, packed, args)
        out, key_pad = embed_concat_pe_fwd(dense_ids, [t.detach() for t in tables], pe.detach(), scale, rate, seed, dtype, packed,
                                           combine)
        ctx.save_for_backward(*ids, *tables)
        ctx.n, ctx.scale, ctx.rate, ctx.seed = n, scale, rate, seed
        ctx.mark_non_differentiable(key_pad)
        ctx.set_materialize_grads(False)       # (or autograd fills a zero "gradient" of key_pad's size every step)
        return out, key_pad

    @staticmethod
    def backward(ctx, dout, _):
        saved = ctx.saved_tensors
        ids, tables = list(saved[:ctx.n]), list(saved[ctx.n:])
        flush_pending_dw(getattr(tables[0], '_b4c_ctx', None))
        if dout is None:
            return (None,) * len(ctx.needs_input_grad)
        dout = dout.reshape(ids[0].shape[0], ids[0].shape[1], -1).contiguous()
        return _embed_stage_bwd(ctx, ids, tables, dout, ctx.rate, ctx.seed)


class EmbedLNFn(torch.autograd.Function):
    """The paper's input stage (no reference counterpart): drop(LayerNorm(scale * rows + PE)), one kernel each way
    (b4c_embed_ln_fwd / _bwd).  apply(pe, gamma, beta, scale, rate, seed, dtype, packed, combine, n, *ids, *tables), as EmbedFn's.
    The tables' and a learned pe's gradients are EmbedFn's kernels on the pre-norm gradient, at rate 0."""

    @staticmethod
    def forward(ctx, pe, gamma, beta, scale, rate, seed, dtype, packed, combine, n, *args):
        dense_ids, ids, tables = _embed_stage_fwd(ctx, pe, n, packed, args)
        out, key_pad, stats = embed_ln_fwd(dense_ids, [t.detach() for t in tables], pe.detach(), scale, gamma.detach(), beta.detach(),
                                           rate, seed, dtype, packed, combine)
        ctx.save_for_backward(*ids, *tables, *(dense_ids if packed is not None else ()), stats)
        ctx.n, ctx.scale, ctx.rate, ctx.seed, ctx.packed, ctx.combine = n, scale, rate, seed, packed, combine
        ctx.norm = (gamma, beta)
        ctx.mark_non_differentiable(key_pad)
        ctx.set_materialize_grads(False)       # (or autograd fills a zero "gradient" of key_pad's size every step)
        return out, key_pad

    @staticmethod
    def backward(ctx, dout, _):
        saved, n = ctx.saved_tensors, ctx.n
        ids, tables, stats = list(saved[:n]), list(saved[n:2 * n]), saved[-1]
        dense_ids = list(saved[2 * n:3 * n]) if ctx.packed is not None else ids
        flush_pending_dw(getattr(tables[0], '_b4c_ctx', None))
        if dout is None:
            return (None,) * len(ctx.needs_input_grad)
        gamma, beta = ctx.norm
        gctx, gsinks = grad_sinks(gamma, beta)
        dpre, _, _ = embed_ln_bwd(dense_ids, [t.detach() for t in tables], ctx.pe.detach(), ctx.scale, gamma.detach(), stats,
                                  dout.reshape(-1, dout.shape[-1]).contiguous(), ctx.rate, ctx.seed, ctx.packed, ctx.combine,
                                  into=gsinks)
        _ready(gamma, beta)
        dpre = dpre.reshape(ids[0].shape[0], ids[0].shape[1], -1)
        return _embed_stage_bwd(ctx, ids, tables, dpre, 0.0, 0, lead=(None, None) if gctx is not None else gsinks)


class DenseActLNFn(torch.autograd.Function):
    """The paper's masked-item transform (no reference counterpart): LayerNorm(act(x W + b)), act = relu or a GELU (`act`:
    B4C_ACT_*).  apply(x, w, b, gamma, beta, pack, act, training).  A GELU saves the pre-activation beside the activation, as
    FFNBlockFn does; the LayerNorm backward applies act' as it stores its dx."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, pk, act, training):
        wt, _, bias = pk.get(x.dtype, x.shape[1], training)
        relu = act == L.ACT_RELU
        u = torch.empty(x.shape[0], pk.Np, dtype=x.dtype, device=x.device) if (training and not relu) else None
        with _timed('head_mlp_fwd'):
            a = gemm_nt(x, wt, pk.Np, bias, act=act, pre=u)
            out, stats = layernorm_fwd(a, gamma.detach(), beta.detach())
        if training:
            ctx.save_for_backward(x, a, stats, *(() if relu else (u,)))
            ctx.pk, ctx.act, ctx.params = pk, act, (w, b, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, a, stats = ctx.saved_tensors[:3]
        w, b, gamma, beta = ctx.params
        pk = ctx.pk
        actx, sinks = grad_sinks(*ctx.params)
        gw, gb, ggam, gbet = sinks
        gate = a if ctx.act == L.ACT_RELU else ctx.saved_tensors[3]
        du, _, _ = layernorm_bwd(_rows_ok(dout, a.dtype).contiguous(), a, stats, gamma.detach(), into=(ggam, gbet), gate=gate,
                                 gate_act=ctx.act)
        _ready(gamma, beta)
        _, wc, _ = pk.get(x.dtype, x.shape[1], True)
        queue_dw(actx, x, du, pk.K, pk.N, [gw], [gb], (w, b))
        with _timed('head_mlp_dx'):
            dx = gemm_nt(du, wc, x.shape[1])
        flush_pending_dw(actx)
        return sink_returns(ctx, (dx,), actx, sinks)


def _residual_ln_fwd(a, wt, bias, x, gamma, beta, rate, seed, training):
    """The tail of an encoder half: LayerNorm(x + drop(a @ wt^T + bias)) -> (z, out, stats); z and stats only in training.  bf16 up
    to d_model 256: the GEMM does it in its epilogue (gemm_ln_supported)."""
    d = x.shape[1]
    rate = rate if training else 0.0
    if gemm_ln_supported(a, d):
        return gemm_nt_add_ln(a, wt, bias, x, gamma.detach(), beta.detach(), rate, seed, save=training)
    y = gemm_nt(a, wt, d, bias)
    return add_dropout_layernorm_fwd(x, y, gamma.detach(), beta.detach(), rate, seed, save=training)


def _attn_tail_bwd(dout, z, stats, gamma, rate, seed, o, wc_o, params, actx, sinks, dxdw):
    """Backward of _residual_ln_fwd behind an attention kernel -> (dz, d_o): the gradient of the residual branch and of the
    attention output o.  params / sinks: the block's ten (wq, bq, wk, bk, wv, bv, wo, bo, gamma, beta) and their sinks; the
    gradients of wo, bo, gamma, beta are added here.  dxdw: the output projection may take gemm_dxdw (the full block alone)."""
    wo, bo = params[6:8]
    gwo, gbo, ggam, gbet = sinks[6:]
    d = z.shape[1]
    routes = _arena_routes(actx)
    if routes and fused_attn_out_bwd and attn_out_bwd_supported(o, z):
        dz, d_o = attn_out_bwd(dout.contiguous(), z, stats, gamma.detach(), rate, seed, o, wc_o, gwo, gbo, ggam, gbet)
        _ready(wo, bo)
        return dz, d_o
    dz, dy, _, _ = add_dropout_layernorm_bwd(dout.contiguous(), z, stats, gamma.detach(), rate, seed, into=(ggam, gbet))
    if dxdw and routes and fused_dxdw >= 3 and dxdw_supported(o, dy, 1):
        d_o = gemm_dxdw(o, dy, wc_o, [gwo], [gbo])
        _ready(wo, bo)
    else:
        queue_dw(actx, o, dy, d, d, [gwo], [gbo], (wo, bo))
        d_o = gemm_nt(dy, wc_o, d)
    return dz, d_o


class AttnBlockFn(torch.autograd.Function):
    """R8 + first half of R10: LN1(x + drop(MHA(x))).  x: [T, d] in the compute dtype.
    attn_rate, attn_seed: dropout on the attention probabilities (attn_fwd; no reference counterpart), applied as given.
    causal: left-to-right attention (attn_fwd(causal=True))."""

    @staticmethod
    def forward(ctx, x, key_pad, wq, bq, wk, bk, wv, bv, wo, bo, gamma, beta, pk_qkv, pk_o, B, S, H, rate, seed, training, cu=None,
                attn_rate=0.0, attn_seed=0, causal=False):
        T_tok, d = x.shape
        dh = d // H
        wt_qkv, _, b_qkv = pk_qkv.get(x.dtype, d, training)
        wt_o, _, b_o = pk_o.get(x.dtype, d, training)
        with _timed('qkv_fwd'):
            qkv = gemm_nt(x, wt_qkv, 3 * d, b_qkv)
        # (without attention dropout: attn_fwd / attn_bwd are called as they have always been, without the keywords)
        attn_drop = {'rate': attn_rate, 'seed': attn_seed} if attn_rate > 0 else {}
        if causal:              # (likewise: a bidirectional block makes the calls it makes without this keyword)
            attn_drop['causal'] = True
        with _timed('attn_fwd'):
            o, lse = attn_fwd(qkv, key_pad, B, S, H, dh, cu, **attn_drop)
        z, out, stats = _residual_ln_fwd(o, wt_o, b_o, x, gamma, beta, rate, seed, training)
        if training:
            ctx.save_for_backward(x, key_pad, qkv, o, lse, z, stats, gamma)
            ctx.pk = (pk_qkv, pk_o)
            ctx.dims = (B, S, H, dh, rate, seed)
            ctx.cu = cu
            ctx.attn_drop = attn_drop
            ctx.params = (wq, bq, wk, bk, wv, bv, wo, bo, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, key_pad, qkv, o, lse, z, stats, gamma = ctx.saved_tensors
        pk_qkv, pk_o = ctx.pk
        B, S, H, dh, rate, seed = ctx.dims
        wq, bq, wk, bk, wv, bv = ctx.params[:6]
        d = H * dh
        actx, sinks = grad_sinks(*ctx.params)
        gwq, gbq, gwk, gbk, gwv, gbv = sinks[:6]
        _, wc_o, _ = pk_o.get(x.dtype, d, True)
        _, wc_qkv, _ = pk_qkv.get(x.dtype, d, True)
        dz, d_o = _attn_tail_bwd(dout, z, stats, gamma, rate, seed, o, wc_o, ctx.params, actx, sinks, dxdw=True)
        with _timed('attn_bwd'):
            dqkv = attn_bwd(qkv, key_pad, o, d_o, lse, B, S, H, dh, ctx.cu, actx, **ctx.attn_drop)
        if _arena_routes(actx) and fused_dxdw and dxdw_supported(x, dqkv, 3, residual=dz):
            # dX and dW | db of the fused Q | K | V projection in one pass over dqkv (csrc/gemm_dxdw.hip)
            dx = gemm_dxdw(x, dqkv, wc_qkv, [gwq, gwk, gwv], [gbq, gbk, gbv], residual=dz)
            _ready(wq, bq, wk, bk, wv, bv)
        else:
            queue_dw(actx, x, dqkv, d, 3 * d, [gwq, gwk, gwv], [gbq, gbk, gbv], (wq, bq, wk, bk, wv, bv))
            dx = gemm_nt(dqkv, wc_qkv, d, residual=dz)
        _ready(*ctx.params[8:])
        flush_pending_dw(actx)      # this layer's four weight gradients (two queued by FFNBlockFn.backward) in one launch
        return sink_returns(ctx, (dx, None), actx, sinks)


def attn_keep_mask(seed, B, H, S_arg, rate):
    """Host regeneration of an attention-dropout keep-mask (tests): bool [B, H, S_arg, S_arg], element (b, h, q, k) kept iff
    b4c_attn_keep(seed, b, h, q, k, H, S_arg, rate): element ((b*H + h) * S_arg + q) * S4 + k of keep_mask's stream, S4 = S_arg
    rounded up to a multiple of 4.  S_arg: the pitch of the launch (S, or the packed layout's max_len); q, k count inside the
    sequence."""
    S4 = (S_arg + 3) // 4 * 4
    m = torch.from_numpy(keep_mask(seed, B * H * S_arg * S4, rate))
    return m.view(B, H, S_arg, S4)[..., :S_arg].contiguous()


def rows_add_(dst, idx, src):
    """dst[idx[r]] += src[r] for idx[r] >= 0 (distinct indices)."""
    if src.shape[0] == 0:
        return dst
    L.check(L.lib().b4c_rows_add(_p(dst), dst.stride(0), _p(idx), _p(src), src.stride(0), src.shape[0], src.shape[1],
                                 dt_code(dst.dtype), dt_code(src.dtype), _st()), 'rows_add')
    return dst


# Cloze path: the last encoder layer runs for the [MASK] rows only (MQAttnBlockFn); B4C_MQ_LAST_LAYER=0 computes the full layer
mq_last_layer = os.environ.get('B4C_MQ_LAST_LAYER', '1') != '0'
# ... also in training with attention_dropout_rate > 0: the masked-query kernels draw the full layer's masks for their rows
# (b4c_attn_mq_*_drop).  Off (B4C_MQ_ATTN_DROPOUT=1 switches it on): such a pass takes the full last layer and gathers its rows,
# Encoder.rows_supported's answer; Encoder.rows_route is the route with this switch applied.
mq_attn_dropout = os.environ.get('B4C_MQ_ATTN_DROPOUT', '0') == '1'
# ... and for a causal encoder (attention='causal'): the masked-query kernels' causal form (b4c_attn_mq_*_ex, B4C_ATTN_CAUSAL), every
# query row over the keys up to its own position.  Off (B4C_MQ_CAUSAL=1 switches it on): a causal encoder takes the full last layer
# and gathers its rows, Encoder.rows_supported's answer; Encoder.rows_route is the route with this switch applied too.
mq_causal = os.environ.get('B4C_MQ_CAUSAL', '0') == '1'


class MQAttnBlockFn(torch.autograd.Function):
    """The attention half of the LAST encoder layer for the query rows `midx` only: LN1(x_m + drop(MHA(x)_m)).
    Every other row of that layer's output is never read on the Cloze path (clickstream_transformer.py:281-295 keeps the
    [MASK] rows); keys and values still come from every token.
      x [T, d] (all tokens), midx [R] int32 (token row of each query row, -1 = unused row), moff [B+1] (query rows of
      sequence b), cu [B+1] (its token rows), key_pad [T] or None  ->  out1_m [R, d].
    attn_rate > 0: dropout on the attention probabilities, the masks AttnBlockFn draws with attn_seed for the rows midx.
    causal (a trailing argument a bidirectional caller does not pass): the last layer of a causal encoder, each query row over the
    keys up to its own position (midx is the kernels' q_rows either way)."""

    @staticmethod
    def forward(ctx, x, midx, moff, cu, key_pad, wq, bq, wk, bk, wv, bv, wo, bo, gamma, beta, pk_qkv, pk_o, B, max_len, H, rate, seed,
                training, attn_rate=0.0, attn_seed=0, causal=False):
        T_tok, d = x.shape
        dh = d // H
        R = midx.shape[0]
        wt_qkv, _, b_qkv = pk_qkv.get(x.dtype, d, training)
        wt_o, _, b_o = pk_o.get(x.dtype, d, training)
        kv = gemm_nt(x, wt_qkv[d:3 * d], 2 * d, b_qkv[d:3 * d])            # K | V of every token
        x_m = gather_rows(x, midx, R)
        q_m = gemm_nt(x_m, wt_qkv[:d], d, b_qkv[:d])
        o_m, lse = attn_mq_fwd(q_m, kv, cu, moff, B, max_len, H, dh, key_pad, midx, attn_rate, attn_seed, **({'causal': True} if causal else {}))
        z, out, stats = _residual_ln_fwd(o_m, wt_o, b_o, x_m, gamma, beta, rate, seed, training)
        if training:
            ctx.save_for_backward(x, x_m, midx, moff, cu, key_pad, q_m, kv, o_m, lse, z, stats, gamma)
            ctx.pk = (pk_qkv, pk_o)
            ctx.dims = (B, max_len, H, dh, rate, seed, attn_rate, attn_seed)
            ctx.causal = bool(causal)
            ctx.params = (wq, bq, wk, bk, wv, bv, wo, bo, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, x_m, midx, moff, cu, key_pad, q_m, kv, o_m, lse, z, stats, gamma = ctx.saved_tensors
        pk_qkv, pk_o = ctx.pk
        B, max_len, H, dh, rate, seed, attn_rate, attn_seed = ctx.dims
        wq, bq, wk, bk, wv, bv = ctx.params[:6]
        d = H * dh
        actx, sinks = grad_sinks(*ctx.params)
        gwq, gbq, gwk, gbk, gwv, gbv = sinks[:6]
        _, wc_o, _ = pk_o.get(x.dtype, d, True)
        _, wc_qkv, _ = pk_qkv.get(x.dtype, d, True)
        dz, d_o = _attn_tail_bwd(dout, z, stats, gamma, rate, seed, o_m, wc_o, ctx.params, actx, sinks, dxdw=False)
        dq, dkv = attn_mq_bwd(q_m, kv, cu, moff, o_m, d_o, lse, B, max_len, H, dh, key_pad, midx, attn_rate, attn_seed,
                              **({'causal': True} if ctx.causal else {}))
        queue_dw(actx, x_m, dq, d, d, [gwq], [gbq], (wq, bq))
        flush_pending_dw(actx)                  # (the query-row problems have R rows, the key / value problem T)
        dx_m = gemm_nt(dq, wc_qkv[:, :d], d, residual=dz, out_dtype=torch.float32)      # query rows: through Wq + the residual branch (kept in fp32 until it joins dx)
        # every token: through Wk | Wv
        if _arena_routes(actx) and fused_dxdw >= 2 and dxdw_supported(x, dkv, 2):
            dx = gemm_dxdw(x, dkv, wc_qkv[:, d:3 * d], [gwk, gwv], [gbk, gbv])
            _ready(wk, bk, wv, bv)
        else:
            queue_dw(actx, x, dkv, d, 2 * d, [gwk, gwv], [gbk, gbv], (wk, bk, wv, bv))
            dx = gemm_nt(dkv, wc_qkv[:, d:3 * d], d)
        rows_add_(dx, midx, dx_m)
        _ready(*ctx.params[8:])
        flush_pending_dw(actx)
        return sink_returns(ctx, (dx, None, None, None, None), actx, sinks)


class FFNBlockFn(torch.autograd.Function):
    """R9 + second half of R10: LN2(x + drop(act(x W1 + b1) W2 + b2)), act = relu (the reference) or a GELU (`act`: B4C_ACT_*,
    no reference counterpart).  A GELU block saves the pre-activation u beside h = gelu(u) -- one GEMM launch writes both --
    and its backward gates with gelu'(u); the fused kernels b4c_ffn_fwd / b4c_ffn_bwd are ReLU kernels and are not taken.  With
    `fused_ffn_gelu` (off by default) a GELU block of the fused shape takes b4c_ffn_act_fwd / b4c_ffn_act_bwd instead."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, pk1, pk2, rate, seed, training, act=L.ACT_RELU):
        T_tok, d = x.shape
        wt1, _, bb1 = pk1.get(x.dtype, d, training)
        Fp = pk1.Np
        wt2, _, bb2 = pk2.get(x.dtype, Fp, training)
        relu = act == L.ACT_RELU
        # a GELU block in training: the pre-activation leaves the first GEMM beside h (inference saves nothing extra)
        fused_act = not relu and fused_ffn_gelu
        if relu and fused_ffn_fwd and ffn_fwd_supported(x, Fp):
            h, z, out, stats = ffn_fwd(x, wt1, bb1, wt2, bb2, gamma.detach(), beta.detach(), pk1.N, Fp, rate if training else 0.0, seed,
                                       save=training)
        elif fused_act and fused_ffn_fwd and ffn_fwd_supported(x, Fp):
            h, u, z, out, stats = ffn_act_fwd(x, wt1, bb1, wt2, bb2, gamma.detach(), beta.detach(), pk1.N, Fp, act,
                                              rate if training else 0.0, seed, save=training)
        else:
            u = torch.empty(T_tok, Fp, dtype=x.dtype, device=x.device) if (training and not relu) else None
            h = gemm_nt(x, wt1, Fp, bb1, act=act, pre=u)
            z, out, stats = _residual_ln_fwd(h, wt2, bb2, x, gamma, beta, rate, seed, training)
        if training:
            ctx.save_for_backward(x, h, z, stats, gamma, *(() if relu else (u,)))
            ctx.pk = (pk1, pk2)
            ctx.dims = (rate, seed)
            ctx.act = act
            ctx.params = (w1, b1, w2, b2, gamma, beta)
            # A model of the fused kernels' shape runs the head's dW sweep in the foreground (_background_dw_for) -- decided by the
            # SHAPE, whatever the batch's row count, so that it agrees with background_dw_expected(), by which callers order their
            # gradient arenas (a background sweep's gradient completes last and belongs to the reducer's last bucket)
            if (relu or fused_act) and fused_ffn_bwd and ffn_bwd_shape_ok(x, h, z):
                actx = arena_context(w1, b1, w2, b2, gamma, beta)
                if actx is not None:
                    actx.fused_blocks = True
        return out

    @staticmethod
    def backward(ctx, dout):
        x, h, z, stats, gamma = ctx.saved_tensors[:5]
        pk1, pk2 = ctx.pk
        rate, seed = ctx.dims
        relu = ctx.act == L.ACT_RELU
        w1, b1, w2, b2, gam, bet = ctx.params
        d, Fp = x.shape[1], h.shape[1]
        actx, sinks = grad_sinks(*ctx.params)
        gw1, gb1, gw2, gb2, ggam, gbet = sinks
        _, wc1, _ = pk1.get(x.dtype, d, True)
        _, wc2, _ = pk2.get(x.dtype, Fp, True)
        if relu and _arena_routes(actx) and fused_ffn_bwd and ffn_bwd_supported(x, h, z):
            dx = ffn_bwd(dout.contiguous(), z, stats, gamma.detach(), rate, seed, h, x, wc2, wc1, pk1.N, gw1, gb1, gw2, gb2, ggam, gbet)
            _ready(w1, b1, w2, b2, gam, bet)
            return sink_returns(ctx, (dx,), actx, sinks)
        if not relu and fused_ffn_gelu and _arena_routes(actx) and fused_ffn_bwd and ffn_bwd_supported(x, h, z):
            dx = ffn_act_bwd(dout.contiguous(), z, stats, gamma.detach(), rate, seed, ctx.act, h, ctx.saved_tensors[5], x, wc2, wc1,
                             pk1.N, gw1, gb1, gw2, gb2, ggam, gbet)
            _ready(w1, b1, w2, b2, gam, bet)
            return sink_returns(ctx, (dx,), actx, sinks)
        dz, dy, _, _ = add_dropout_layernorm_bwd(dout.contiguous(), z, stats, gamma.detach(), rate, seed, into=(ggam, gbet))
        queue_dw(actx, h, dy, pk2.K, d, [gw2], [gb2], (w2, b2))
        # ReLU: the saved activation's sign; GELU: gelu'(u) of the saved pre-activation (gelu is not invertible)
        dh = gemm_nt(dy, wc2, Fp, gate=h) if relu else gemm_nt(dy, wc2, Fp, gate=ctx.saved_tensors[5], gate_act=ctx.act)
        queue_dw(actx, x, dh, d, pk1.N, [gw1], [gb1], (w1, b1))
        dx = gemm_nt(dh, wc1, d, residual=dz)
        _ready(gam, bet)
        return sink_returns(ctx, (dx,), actx, sinks)


# ---- pre-LN encoder halves (norm='pre'):  x' = x + drop(sublayer(LN(x; gamma, beta))),  no reference counterpart ---------------
# The residual stream x is what a half takes and returns; the normalised rows n = LN(x) and their stats ride beside it.  The
# forward needs no launch of its own: the tail kernel of the post-LN half (_residual_ln_fwd) writes z = x + drop(a W^T + b) AND
# LN(z), so with the NEXT norm's gamma / beta its two outputs are the stream and the next half's normalised input -- the LayerNorm
# parameters shift by one place, one layernorm_fwd in front of the first layer starts the chain and the last half is given the
# encoder's final norm.  n and stats are therefore NON-differentiable companions: the half that consumes them owns their LayerNorm
# backward and adds it to the stream's gradient (layernorm_bwd_add), with its own gamma / beta sinks.  The four persistent
# kernels (b4c_ffn_bwd, b4c_ffn_act_bwd, b4c_attn_out_bwd, b4c_ffn_fwd / b4c_ffn_act_fwd) are post-LN kernels and are not taken;
# actx.fused_blocks is not set (background_dw_expected(norm='pre')).
#
# The input-gradient step of a half -- dn = dqkv Wqkv^T (dn = dh W1^T) with the weight gradient n^T dqkv (n^T dh), then
# dx = g + LNbwd(dn) -- has three forms.  'pair': b4c_gemm_nt, then b4c_layernorm_bwd_add, the weight gradient queued for the
# layer's grouped launch; it exists everywhere.  'fused': b4c_gemm_nt_ln_bwd_add does both in one pass and dn never reaches memory
# (bf16, d_model <= 256: gemm_ln_bwd_supported), the weight gradient queued as in 'pair'.  'dxdw': the attention half's step takes
# b4c_gemm_dxdw (dn and dW in one pass over dqkv; bf16, d_model 128, an arena, 4,096 rows or more) and b4c_layernorm_bwd_add; its
# feed-forward half, and every shape b4c_gemm_dxdw does not take, runs 'pair'.  B4C_PRE_LN_INPUT_BWD names the form.
pre_ln_input_bwd = os.environ.get('B4C_PRE_LN_INPUT_BWD', 'dxdw')
PRE_LN_INPUT_BWD_FORMS = ('dxdw', 'pair', 'fused')


def _pre_ln_input_form():
    if pre_ln_input_bwd not in PRE_LN_INPUT_BWD_FORMS:
        raise ValueError('pre_ln_input_bwd must be one of %r, got %r' % (PRE_LN_INPUT_BWD_FORMS, pre_ln_input_bwd))
    return pre_ln_input_bwd


def _pre_ln_input_bwd(g_in, wc, x, stats, gamma, g, sinks):
    """dx = g + LNbwd(g_in wc^T; x, stats, gamma) in the 'fused' form where the kernel takes the shape, else as the pair"""
    d = x.shape[1]
    if _pre_ln_input_form() == 'fused' and gemm_ln_bwd_supported(g_in, wc, d):
        return gemm_nt_ln_bwd_add(g_in, wc, x, stats, gamma.detach(), g, into=sinks)[0]
    return layernorm_bwd_add(gemm_nt(g_in, wc, d), x, stats, gamma.detach(), g, into=sinks)[0]


def _pre_ln_tail_fwd(a, wt, bias, x, next_gamma, next_beta, rate, seed):
    """-> (x' = x + drop(a @ wt^T + bias), n' = LN(x'; the next norm), its stats): _residual_ln_fwd in its training form, so that
    the stream is produced in inference too"""
    return _residual_ln_fwd(a, wt, bias, x, next_gamma, next_beta, rate, seed, True)


def _pre_ln_stream_grad(g, dtype, rate, seed):
    """(g as the kernels take it, the sublayer output's gradient drop(g)): the keep rule on e = t * d_model + col, as the forward's"""
    g = _rows_ok(g, dtype).contiguous()
    return g, (dropout(g, rate, seed) if rate > 0 else g)


class PreLNAttnBlockFn(torch.autograd.Function):
    """The attention half of a pre-LN layer.  apply(x, <the ten parameters of AttnBlockFn: gamma, beta = THIS half's norm>, n, stats,
    key_pad, next_gamma, next_beta, pk_qkv, pk_o, B, S, H, rate, seed, training, cu, attn_rate, attn_seed, causal)
    -> (x', n', stats'):  n = LN(x; gamma, beta) and stats as the previous tail (or layernorm_fwd) left them;
    x' = x + drop(MHA(n, n, n) Wo + bo), n' = LN(x'; next_gamma, next_beta).  Only x' is differentiable, and only in x."""

    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, wv, bv, wo, bo, gamma, beta, n, stats, key_pad, next_gamma, next_beta, pk_qkv, pk_o, B, S, H,
                rate, seed, training, cu=None, attn_rate=0.0, attn_seed=0, causal=False):
        T_tok, d = x.shape
        dh = d // H
        wt_qkv, _, b_qkv = pk_qkv.get(x.dtype, d, training)
        wt_o, _, b_o = pk_o.get(x.dtype, d, training)
        with _timed('qkv_fwd'):
            qkv = gemm_nt(n, wt_qkv, 3 * d, b_qkv)
        attn_drop = {'rate': attn_rate, 'seed': attn_seed} if attn_rate > 0 else {}
        if causal:
            attn_drop['causal'] = True
        with _timed('attn_fwd'):
            o, lse = attn_fwd(qkv, key_pad, B, S, H, dh, cu, **attn_drop)
        z, out, stats2 = _pre_ln_tail_fwd(o, wt_o, b_o, x, next_gamma, next_beta, rate, seed)
        if training:
            ctx.save_for_backward(x, n, stats, key_pad, qkv, o, lse, gamma)
            ctx.pk = (pk_qkv, pk_o)
            ctx.dims = (B, S, H, dh, rate, seed)
            ctx.cu = cu
            ctx.attn_drop = attn_drop
            ctx.params = (wq, bq, wk, bk, wv, bv, wo, bo, gamma, beta)
        ctx.mark_non_differentiable(out, stats2)
        return z, out, stats2

    @staticmethod
    def backward(ctx, g, _dn, _dstats):
        x, n, stats, key_pad, qkv, o, lse, gamma = ctx.saved_tensors
        pk_qkv, pk_o = ctx.pk
        B, S, H, dh, rate, seed = ctx.dims
        wq, bq, wk, bk, wv, bv, wo, bo, gam, bet = ctx.params
        d = H * dh
        actx, sinks = grad_sinks(*ctx.params)
        gwq, gbq, gwk, gbk, gwv, gbv, gwo, gbo, ggam, gbet = sinks
        routes = _arena_routes(actx)
        _, wc_o, _ = pk_o.get(x.dtype, d, True)
        _, wc_qkv, _ = pk_qkv.get(x.dtype, d, True)
        g, dy = _pre_ln_stream_grad(g, x.dtype, rate, seed)
        if routes and fused_dxdw >= 3 and dxdw_supported(o, dy, 1):
            d_o = gemm_dxdw(o, dy, wc_o, [gwo], [gbo])
            _ready(wo, bo)
        else:
            queue_dw(actx, o, dy, d, d, [gwo], [gbo], (wo, bo))
            d_o = gemm_nt(dy, wc_o, d)
        with _timed('attn_bwd'):
            dqkv = attn_bwd(qkv, key_pad, o, d_o, lse, B, S, H, dh, ctx.cu, actx, **ctx.attn_drop)
        # the weight-gradient operand is the normalised rows; the input gradient is the stream's plus the norm's backward
        if _pre_ln_input_form() == 'dxdw' and routes and fused_dxdw and dxdw_supported(n, dqkv, 3):
            dn = gemm_dxdw(n, dqkv, wc_qkv, [gwq, gwk, gwv], [gbq, gbk, gbv])
            _ready(wq, bq, wk, bk, wv, bv)
            dx, _, _ = layernorm_bwd_add(dn, x, stats, gamma.detach(), g, into=(ggam, gbet))
        else:
            queue_dw(actx, n, dqkv, d, 3 * d, [gwq, gwk, gwv], [gbq, gbk, gbv], (wq, bq, wk, bk, wv, bv))
            dx = _pre_ln_input_bwd(dqkv, wc_qkv, x, stats, gamma, g, (ggam, gbet))
        _ready(gam, bet)
        flush_pending_dw(actx)      # this layer's weight gradients (two queued by PreLNFFNBlockFn.backward) in one launch
        return sink_returns(ctx, (dx,), actx, sinks)


class PreLNFFNBlockFn(torch.autograd.Function):
    """The feed-forward half of a pre-LN layer.  apply(x, w1, b1, w2, b2, gamma, beta, n, stats, next_gamma, next_beta, pk1, pk2,
    rate, seed, training, act) -> (x', n', stats'):  x' = x + drop(act(n W1 + b1) W2 + b2) with n = LN(x; gamma, beta) given,
    n' = LN(x'; next_gamma, next_beta).  A GELU saves the pre-activation beside the activation, as FFNBlockFn does."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, n, stats, next_gamma, next_beta, pk1, pk2, rate, seed, training,
                act=L.ACT_RELU):
        T_tok, d = x.shape
        wt1, _, bb1 = pk1.get(x.dtype, d, training)
        Fp = pk1.Np
        wt2, _, bb2 = pk2.get(x.dtype, Fp, training)
        relu = act == L.ACT_RELU
        u = torch.empty(T_tok, Fp, dtype=x.dtype, device=x.device) if (training and not relu) else None
        h = gemm_nt(n, wt1, Fp, bb1, act=act, pre=u)
        z, out, stats2 = _pre_ln_tail_fwd(h, wt2, bb2, x, next_gamma, next_beta, rate, seed)
        if training:
            ctx.save_for_backward(x, n, stats, h, gamma, *(() if relu else (u,)))
            ctx.pk = (pk1, pk2)
            ctx.dims = (rate, seed)
            ctx.act = act
            ctx.params = (w1, b1, w2, b2, gamma, beta)
        ctx.mark_non_differentiable(out, stats2)
        return z, out, stats2

    @staticmethod
    def backward(ctx, g, _dn, _dstats):
        x, n, stats, h, gamma = ctx.saved_tensors[:5]
        pk1, pk2 = ctx.pk
        rate, seed = ctx.dims
        relu = ctx.act == L.ACT_RELU
        w1, b1, w2, b2, gam, bet = ctx.params
        d, Fp = x.shape[1], h.shape[1]
        actx, sinks = grad_sinks(*ctx.params)
        gw1, gb1, gw2, gb2, ggam, gbet = sinks
        _, wc1, _ = pk1.get(x.dtype, d, True)
        _, wc2, _ = pk2.get(x.dtype, Fp, True)
        g, dy = _pre_ln_stream_grad(g, x.dtype, rate, seed)
        queue_dw(actx, h, dy, pk2.K, d, [gw2], [gb2], (w2, b2))
        dh = gemm_nt(dy, wc2, Fp, gate=h) if relu else gemm_nt(dy, wc2, Fp, gate=ctx.saved_tensors[5], gate_act=ctx.act)
        queue_dw(actx, n, dh, d, pk1.N, [gw1], [gb1], (w1, b1))
        dx = _pre_ln_input_bwd(dh, wc1, x, stats, gamma, g, (ggam, gbet))
        _ready(gam, bet)
        return sink_returns(ctx, (dx,), actx, sinks)


class PreLNFinalNormFn(torch.autograd.Function):
    """The encoder's final norm.  apply(x, gamma, beta, n, stats) -> n = LN(x; gamma, beta), which the last half's tail has already
    computed: nothing is launched in the forward; the backward is layernorm_bwd (the stream ends here: no residual term)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, n, stats, training):
        if training:
            ctx.save_for_backward(x, stats, gamma)
            ctx.params = (gamma, beta)
        return n.view_as(n)

    @staticmethod
    def backward(ctx, dout):
        x, stats, gamma = ctx.saved_tensors
        actx, sinks = grad_sinks(*ctx.params)
        dx, _, _ = layernorm_bwd(_rows_ok(dout, x.dtype).contiguous(), x, stats, gamma.detach(), into=tuple(sinks))
        _ready(*ctx.params)
        return sink_returns(ctx, (dx,), actx, sinks)


class MLPFn(torch.autograd.Function):
    """Chain of dense layers (relu on all but the last): the SoftMaxHead's trunk + vocabulary
    projection (R12, logits).  apply(x, packs, training, out_fp32, relu_last, *[k0, b0, k1, b1, ...]); out_fp32: the last layer's
    output in fp32; relu_last: every layer (also the last) is followed by relu -- the head's trunk alone."""

    @staticmethod
    def forward(ctx, x, packs, training, out_fp32, relu_last, *params):
        acts = [x]
        n = len(packs)
        for i, pk in enumerate(packs):
            a = acts[-1]
            wt, _, bias = pk.get(x.dtype, a.shape[1], training)
            last = i == n - 1
            odt = torch.float32 if (last and out_fp32) else a.dtype
            with _timed('vocab_proj_fwd' if last else 'head_mlp_fwd'):
                acts.append(gemm_nt(a, wt, pk.Np, bias, act=L.ACT_RELU if (relu_last or not last) else L.ACT_NONE,
                                    out_dtype=odt, out=empty_rows(a.shape[0], pk.Np, odt, a.device)))
        if training:
            ctx.save_for_backward(*(acts if relu_last else acts[:-1]))
            ctx.packs = packs
            ctx.params = params
            ctx.relu_last = relu_last
        return acts[-1]

    @staticmethod
    def backward(ctx, dlogits):
        acts = ctx.saved_tensors
        packs = ctx.packs
        g = dlogits
        if g.dtype != acts[0].dtype:
            g = g.to(acts[0].dtype)
        if ctx.relu_last:
            if g.is_cuda and g.numel() % 8 == 0 and g.dtype == acts[-1].dtype:
                g = relu_gate(g, acts[-1])
            else:
                g = g * (acts[-1] > 0).to(g.dtype)
        g = _rows_ok(g, acts[0].dtype)      # a pitched [R, Vp] view (empty_rows) is taken as it is
        actx, sinks = grad_sinks(*ctx.params)
        for i in range(len(packs) - 1, -1, -1):
            a = acts[i]
            pk = packs[i]
            _, wc, _ = pk.get(a.dtype, a.shape[1], True)
            last = i == len(packs) - 1
            # (in an arena the layers' weight gradients are queued and go out as one grouped launch below)
            queue_dw(actx, a, g, pk.K, pk.N, [sinks[2 * i]], [sinks[2 * i + 1]], ctx.params[2 * i:2 * i + 2])
            with _timed('vocab_proj_dx' if last else 'head_mlp_dx'):
                g = gemm_nt(g, wc, a.shape[1], gate=a if i > 0 else None)
        flush_pending_dw(actx)
        return sink_returns(ctx, (g, None, None, None, None), actx, sinks)


# Vocabulary-head weight gradient BESIDE the encoder backward.  The dW sweep is MFMA / VALU bound and leaves HBM idle;
# the encoder backward is HBM bound and leaves the matrix pipes idle; nothing in backward consumes the sweep's result.
# As a plain second-stream launch the two only time-slice the CUs (the sweep's 512-thread workgroups hold 2 x 212 registers
# per SIMD: nothing else fits beside them; 10.78 -> 10.71 ms).  What shares the CUs is the BACKGROUND form of the sweep
# (b4c_vocab_ce_dw_sweep, background_workgroups > 0): one wave per SIMD, at most one workgroup per CU, cut into pieces
# that start in the windows BETWEEN the resident attention backward kernels -- those take a whole CU's LDS (146 KB) and
# cannot start on a CU that holds a sweep workgroup.  A piece is launched on the side stream right after every attention
# backward launch (ops.attn_bwd -> _background_kick); how many such launches a backward pass has is learned from the
# previous pass.  The main stream joins, and the gradient is announced to a reducer, when backward ends (join_side_work).
# B4C_OVERLAP_DW=0 switches it off (the sweep then runs in the foreground, first thing in backward), =1 forces it on.
# Unset (None): decided per model.  The fused backward kernels of the d_model = 128 encoder (b4c_ffn_bwd, b4c_gemm_dxdw) hold a
# whole CU like the resident attention backward -- 97 - 145 KB of LDS, 2 x 255 registers per SIMD lane -- so a background sweep
# finds no CU to share and the two only block each other (C2, interleaved on one box: fused + foreground 8.92 - 9.00 ms, five
# kernels + background 9.02 - 9.04, fused + background 9.18 - 9.25, five kernels + foreground 9.59).  A model whose feed-forward
# blocks take the fused backward runs the sweep in the foreground; every other model keeps the background form.
overlap_vocab_dw = {'1': True, '0': False}.get(os.environ.get('B4C_OVERLAP_DW', ''), None)


def background_dw_expected(d_model, dff, dtype, ffn_activation='relu', norm='post'):
    """Will a model of this shape run the vocabulary head's dW sweep as a background job (see overlap_vocab_dw)?
    (b4c_ffn_bwd is a ReLU kernel: a GELU model takes a fused backward, b4c_ffn_act_bwd, only with `fused_ffn_gelu`, which is off
    by default, and otherwise keeps the background sweep.  norm='pre': the fused backward kernels are post-LN kernels, a pre-LN
    model takes none of them and answers as an unfused model does.)"""
    if norm not in ('post', 'pre'):
        raise ValueError("norm must be 'post' or 'pre', got %r" % (norm,))
    if overlap_vocab_dw is not None:
        return overlap_vocab_dw
    if norm == 'pre':
        return True
    return not (fused_ffn_bwd and d_model == 128 and dff <= 128 and dtype == torch.bfloat16 and
                (ffn_activation == 'relu' or fused_ffn_gelu))


def _background_dw_for(actx):
    if overlap_vocab_dw is not None:
        return overlap_vocab_dw
    return not getattr(actx, 'fused_blocks', False)
background_workgroups = int(os.environ.get('B4C_VCE_DW_BG', '0'))      # 0: one per CU of the device
# deterministic_vocab_dw: the projection's dW / db alone in their fixed-order form (see `deterministic`, which includes it and
# is on by default) -- for A/B runs with B4C_DETERMINISTIC=0 (B4C_DETERMINISTIC_DW=1 switches it on).
deterministic_vocab_dw = os.environ.get('B4C_DETERMINISTIC_DW', '0') == '1'


def background_wgs(device):
    """workgroups of a background sweep: ops.background_workgroups, or one per CU of `device` (256 on an MI355X)"""
    if background_workgroups > 0:
        return background_workgroups
    return int(torch.cuda.get_device_properties(device).multi_processor_count)


# the windows' relative lengths: the first one (head trunk + the rows-only last layer + half a layer), one per layer, the last
# one (half a layer + the embedding backward)
background_weights = tuple(float(x) for x in os.environ.get('B4C_VCE_DW_WEIGHTS', '2.2,1.0,0.6').split(','))
_side_streams = {}


def _side_stream(device):
    s = _side_streams.get(device)
    if s is None:
        s = torch.cuda.Stream(device=device)
        _side_streams[device] = s
    return s


def _background_plan(n_tiles, kicks):
    """tile boundaries of the kicks + 1 pieces"""
    w0, wm, wl = background_weights
    w = [w0] + [wm] * max(kicks - 1, 0) + ([wl] if kicks > 0 else [])
    tot, acc, cuts = sum(w), 0.0, [0]
    for x in w[:-1]:
        acc += x
        cuts.append(min(n_tiles, int(round(n_tiles * acc / tot))))
    return cuts + [n_tiles]


def _background_slot(c):
    """One launch opportunity: the queue's head goes out on the side stream, behind everything the main stream has been
    given so far.  The closures still queued are shared out evenly over the opportunities left."""
    left = max(c.slots, 1)
    c.slots = max(c.slots - 1, 0)
    if not c.queue:
        return
    n = max(1, min(len(c.queue), -(-len(c.queue) // left)))
    main = torch.cuda.current_stream()
    side = _side_stream(main.device)
    side.wait_stream(main)
    c.side_launched = main.device
    with torch.cuda.stream(side):
        for _ in range(n):
            c.queue.pop(0)()


def _background_kick(c):
    if c is None or not c.counting:
        return
    c.kicks += 1
    _background_slot(c)


def _background_drain(c):
    """everything queued goes out on the side stream now"""
    if not c.queue:
        return
    main = torch.cuda.current_stream()
    side = _side_stream(main.device)
    side.wait_stream(main)
    c.side_launched = main.device
    with torch.cuda.stream(side):
        while c.queue:
            c.queue.pop(0)()


def join_side_work(c):
    """The current stream waits for everything context `c` issued on the side stream; the gradients that work produced are
    then announced (grad-ready callback), each parameter once and only after EVERY piece has been waited for.  Runs at the
    end of every backward pass that used the side stream (autograd engine callback); optimizers and reducers call it too --
    it is a no-op when nothing is pending."""
    if c is None:
        return
    if c.counting:                  # the pass is over: its number of attention launches is the plan of the next one
        c.counting, c.kicks_expected = False, c.kicks
    _background_drain(c)            # fewer attention launches than planned: what is left of the sweeps goes out now
    c.slots = 0
    done, c.pending[:] = list(c.pending), []
    cur = torch.cuda.current_stream() if done else None
    for ev, _, stream in done:
        stream.wait_event(ev)               # the stream backward ran on (this may be the engine's thread, with another current stream)
        cur.wait_event(ev)
    if c.side_launched is not None:
        if not done:                        # (side-stream work without a closing event: wait for the stream itself)
            torch.cuda.current_stream(c.side_launched).wait_stream(_side_stream(c.side_launched))
        c.side_launched = None
    seen, params = set(), []
    for _, ps, _ in done:
        for p in ps:
            if id(p) not in seen:
                seen.add(id(p))
                params.append(p)
    _ready(*params)


def _dw_pieces(c, h, wt, b, labels_i32, rowscal, V, kernel, bias, cuts):
    """closures for the vocabulary tiles cuts[i] .. cuts[i + 1]; the last one adds the label term and records the event that
    completes the projection's gradient"""
    dW, db = kernel.grad, bias.grad
    side = _side_stream(h.device)
    main = torch.cuda.current_stream(h.device)
    for t in (h, rowscal, labels_i32, wt, b, dW, db):
        if t is not None:
            t.record_stream(side)
    spans = [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1) if cuts[i + 1] > cuts[i]]

    def piece(lo, hi, last):
        def run():
            vocab_ce_dw_sweep(h, wt, b, rowscal, V, dW, db, lo, hi, background_wgs(h.device))
            if last:
                vocab_ce_dw_labels(h, labels_i32, rowscal, V, dW, db)
                c.pending.append((torch.cuda.current_stream().record_event(), (kernel, bias), main))
        return run
    return [piece(lo, hi, i == len(spans) - 1) for i, (lo, hi) in enumerate(spans)]


def _queue_background_dw(c, h, wt, b, labels_i32, rowscal, V, kernel, bias):
    """(inside a backward pass) the dW sweep of the vocabulary head as kicks + 1 background pieces: one now, one behind
    every attention backward launch of this pass"""
    if c.counting or c.queue:
        join_side_work(c)               # a second head on this arena in the same backward pass: finish the first one's sweep first
    cuts = _background_plan((V + 127) // 128, c.kicks_expected)
    c.queue.extend(_dw_pieces(c, h, wt, b, labels_i32, rowscal, V, kernel, bias, cuts))
    c.slots = len(c.queue)
    c.counting, c.kicks = True, 0
    _background_slot(c)
    torch.autograd.Variable._execution_engine.queue_callback(lambda: join_side_work(c))


class VocabCEFn(torch.autograd.Function):
    """R12 + R13 + R14 for training without the (R x V) logits: vocabulary projection, softmax, masked sparse
    CE (mean over valid rows) and their backward, logits recomputed in MFMA accumulators (csrc/vocab_ce.hip).
    apply(h, pack, labels_i32, V, variant, unit_grad, kernel, bias)"""

    @staticmethod
    def forward(ctx, h, pack, labels_i32, V, variant, unit_grad, kernel, bias, poison=None):
        h = h.contiguous()
        wt, _, b = pack.get(h.dtype, h.shape[1], False)
        scale = label_scale(labels_i32, V)                    # [1 / n_valid, n_valid]
        item, dh, rowscal = vocab_ce_fwd(h, wt, b, labels_i32, scale, V, variant)
        ctx.save_for_backward(h, dh, rowscal, labels_i32)
        ctx.pack, ctx.V, ctx.unit_grad = pack, V, unit_grad
        ctx.params = (kernel, bias)
        return sum_scaled(item, scale, poison)

    @staticmethod
    def backward(ctx, g):
        h, dh, rowscal, labels_i32 = ctx.saved_tensors
        kernel, bias = ctx.params
        if not ctx.unit_grad:       # the kernels ran at scale 1/valid in forward: fold the upstream gradient in now
            gf = g.to(torch.float32).reshape(1).contiguous()
            dh_g, rowscal_g = torch.empty_like(dh), torch.empty_like(rowscal)
            L.check(L.lib().b4c_vocab_ce_apply_grad(_p(dh), dh.stride(0), _p(rowscal), _p(gf), _p(dh_g), dh_g.stride(0),
                                                    _p(rowscal_g), dh.shape[0], dh.shape[1], _st()), 'vocab_ce_apply_grad')
            dh, rowscal = dh_g, rowscal_g
        wt, _, b = ctx.pack.get(h.dtype, h.shape[1], False)
        actx, (dW, db) = grad_sinks(kernel, bias)
        off = getattr(ctx.pack, 'tied_offset', None)
        if off is not None:     # tied head: `kernel` is the (rows, K) embedding table; dW [K, V] is added transposed
            dWt = torch.zeros(h.shape[1], ctx.V, dtype=torch.float32, device=h.device)
            vocab_ce_dw(h, wt, b, labels_i32, rowscal, ctx.V, dWt, db)
            transpose_add_(dW[off:off + ctx.V], dWt)
            _tied_table_steps_whole(kernel)
            _ready(bias)        # the table is announced by the embedding backward, which runs last
        elif _arena_routes(actx) and h.is_cuda and _background_dw_for(actx):
            _queue_background_dw(actx, h, wt, b, labels_i32, rowscal, ctx.V, kernel, bias)
        else:
            vocab_ce_dw(h, wt, b, labels_i32, rowscal, ctx.V, dW, db)
            _ready(kernel, bias)
        return sink_returns(ctx, (dh, None, None, None, None, None), actx, (dW, db))


class GatherRowsFn(torch.autograd.Function):
    """R11: rows of the encoder output at the given flat indices (idx < 0 -> zero row)."""

    @staticmethod
    def forward(ctx, src2d, idx, n_out):
        ctx.save_for_backward(idx)
        ctx.n_src = src2d.shape[0]
        return gather_rows(src2d, idx, n_out)

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        return scatter_rows(dout.contiguous(), idx, ctx.n_src), None, None


class FusedSoftmaxCEFn(torch.autograd.Function):
    """R12 tail + R13 + R14 fused for training: softmax over V, masked sparse CE (mean over valid
    rows), and d loss / d logits written in place of the logits (which are consumed)."""

    @staticmethod
    def forward(ctx, logits, labels_i32, V, variant, unit_grad, poison=None):
        scale = label_scale(labels_i32, V)                    # [1 / n_valid, n_valid]
        with _timed('softmax_ce'):
            item = softmax_ce_fwd_bwd_(logits, labels_i32, scale, V, variant)
        ctx.save_for_backward(logits)
        ctx.unit_grad = unit_grad
        return sum_scaled(item, scale, poison)

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        if not ctx.unit_grad:
            dlogits = dlogits * g.to(dlogits.dtype)
        return dlogits, None, None, None, None, None


# --------------------------------------------------------------------------------------
# round 2: the reference's own composition loss(y, model(x)) is differentiable; other heads; MHA in general
# --------------------------------------------------------------------------------------
def dropout(x, rate, seed):
    """keep(seed, e) ? x / (1 - rate) : 0 over the flat element index (its own backward)."""
    _cuda(x)
    x = x.contiguous()
    if x.numel() % 8:
        raise B4CError('dropout: element count %d must be a multiple of 8' % x.numel())
    y = torch.empty_like(x)
    L.check(L.lib().b4c_dropout(_p(x), _p(y), x.numel(), rate, seed, dt_code(x.dtype), _st()), 'dropout')
    return y


class DropoutFn(torch.autograd.Function):
    """Encoder.call's input dropout (transformer.py:263) for an Encoder used on its own."""

    @staticmethod
    def forward(ctx, x, rate, seed):
        ctx.rate, ctx.seed = rate, seed
        return dropout(x, rate, seed)

    @staticmethod
    def backward(ctx, g):
        return dropout(g, ctx.rate, ctx.seed), None, None


def softmax_rows_bwd(probs, g, V):
    R, ld = probs.shape[0], probs.stride(0)
    dx = torch.empty(R, ld, dtype=probs.dtype, device=probs.device)
    if ld != probs.shape[1]:
        dx = dx[:, :probs.shape[1]]
    if R == 0:
        return dx
    L.check(L.lib().b4c_softmax_rows_bwd(_p(probs), ld, _p(g), g.stride(0), _p(dx), ld, R, V, dt_code(probs.dtype), _st()),
            'softmax_rows_bwd')
    return dx


class SoftmaxRowsFn(torch.autograd.Function):
    """Dense(V, softmax)'s activation on materialised logits [R, ld] (head.py:36) with its Jacobian."""

    @staticmethod
    def forward(ctx, logits, V):
        probs = softmax_rows(logits, V)
        ctx.save_for_backward(probs)
        ctx.V = V
        return probs

    @staticmethod
    def backward(ctx, g):
        (probs,) = ctx.saved_tensors
        g = g.to(probs.dtype)
        if g.stride(1) != 1 or g.stride(0) % 8:
            g = g.contiguous()
        return softmax_rows_bwd(probs, g, ctx.V), None


class MaskedSparseCEFn(torch.autograd.Function):
    """MaskedLoss(sparse_categorical_crossentropy)(y_true, y_pred) on PROBABILITIES (losses.py:31-98, main.py:89):
    mean over non-pad rows of the TF-backend sparse CE; differentiable w.r.t. the probabilities.
    apply(probs [R, >=V] with 8-aligned row pitch, labels fp32 [R] (-1 = pad), V, variant)"""

    @staticmethod
    def forward(ctx, probs, labels_f32, V, variant):
        item, nval = sparse_ce_from_probs(probs, labels_f32, V, variant)
        ctx.save_for_backward(probs, labels_f32, nval)
        ctx.V, ctx.variant = V, variant
        return item.sum() / nval[0]

    @staticmethod
    def backward(ctx, g):
        probs, labels_f32, nval = ctx.saved_tensors
        R, ld = probs.shape[0], probs.stride(0)
        gscale = (g.to(torch.float32) / nval[0]).reshape(1).contiguous()
        dp = torch.empty(R, ld, dtype=probs.dtype, device=probs.device)
        if R:
            L.check(L.lib().b4c_sparse_ce_from_probs_bwd(_p(probs), ld, _p(labels_f32), _p(gscale), _p(dp), ld, R, ctx.V,
                                                         ctx.variant, dt_code(probs.dtype), _st()), 'sparse_ce_from_probs_bwd')
        return dp[:, :probs.shape[1]], None, None, None


def sigmoid(x):
    _cuda(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    L.check(L.lib().b4c_sigmoid_fwd(_p(x), _p(y), x.numel(), dt_code(x.dtype), _st()), 'sigmoid_fwd')
    return y


class SigmoidFn(torch.autograd.Function):
    """Dense(activation='sigmoid') of BinaryClassificationHead / MultiLabel_MultiClass_classification (head.py:12,59)."""

    @staticmethod
    def forward(ctx, x):
        y = sigmoid(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = g.to(y.dtype).contiguous()
        dx = torch.empty_like(y)
        L.check(L.lib().b4c_sigmoid_bwd(_p(y), _p(g), _p(dx), y.numel(), dt_code(y.dtype), _st()), 'sigmoid_bwd')
        return dx


def masked_bce(probs, labels_f32, pos_weight=None, want_grad=False):
    """-> (item_loss fp32 [n], sums fp32 [2] = (sum of weighted losses, non-pad count), dprobs fp32 [n] or None)"""
    _cuda(probs)
    n = probs.numel()
    item = torch.empty(n, dtype=torch.float32, device=probs.device)
    sums = torch.zeros(2, dtype=torch.float32, device=probs.device)
    dp = torch.empty(n, dtype=torch.float32, device=probs.device) if want_grad else None
    L.check(L.lib().b4c_masked_bce(_p(probs), _p(labels_f32), float(pos_weight) if pos_weight is not None else 0.0, _p(item),
                                   _p(sums), _p(dp), n, dt_code(probs.dtype), _st()), 'masked_bce')
    return item, sums, dp


class MaskedBCEFn(torch.autograd.Function):
    """MaskedLoss(binary_crossentropy, pos_weight)(y_true, y_pred) (losses.py:31-98): weighted mean over non-pad items,
    divided by (pos_weight + 1) / 2 when a pos_weight is given.  apply(probs (any shape), labels fp32 same count, pos_weight)"""

    @staticmethod
    def forward(ctx, probs, labels_f32, pos_weight):
        p = probs.contiguous()
        _, sums, dp = masked_bce(p, labels_f32, pos_weight, want_grad=True)
        norm = (float(pos_weight) + 1.0) / 2.0 if pos_weight is not None else 1.0
        ctx.save_for_backward(dp, sums)
        ctx.norm, ctx.shape, ctx.dtype = norm, probs.shape, probs.dtype
        return sums[0] / sums[1] / norm

    @staticmethod
    def backward(ctx, g):
        dp, sums = ctx.saved_tensors
        return (dp * (g.to(torch.float32) / sums[1] / ctx.norm)).to(ctx.dtype).view(ctx.shape), None, None


def binary_counts(y_true_f32, y_pred):
    _cuda(y_pred)
    out = torch.zeros(6, dtype=torch.float32, device=y_pred.device)
    yp = y_pred.contiguous()
    L.check(L.lib().b4c_binary_counts(_p(y_true_f32), _p(yp), _p(out), yp.numel(), dt_code(yp.dtype), _st()), 'binary_counts')
    return out


def compact_labels(labels_padded, counts, offsets, cap, flat_idx=None):
    """(B, M) fp32 labels padded with -1 -> int32 [cap] in mask order; entries >= R are -1 (and flat_idx[>= R] = -1)."""
    _cuda(labels_padded)
    B, M = labels_padded.shape
    lab = labels_padded.to(torch.float32).contiguous()
    out = torch.empty(cap, dtype=torch.int32, device=lab.device)
    if M == 0:          # a batch whose label rows are all empty (padded_batch of zero-length arrays, input_pipeline.py:198-214)
        out.fill_(-1)
        if flat_idx is not None:
            flat_idx.fill_(-1)
        return out
    L.check(L.lib().b4c_compact_labels(_p(lab), B, M, _p(counts), _p(offsets), _p(out), _p(flat_idx), cap, _st()),
            'compact_labels')
    return out


def attn_weights(qkv, key_pad, lse, B, S, H, dh, causal=False):
    """causal: lse is that of attn_fwd(causal=True); the weights of the keys behind the query are exactly 0."""
    w = torch.empty(B, H, S, S, dtype=torch.float32, device=qkv.device)
    L.check(L.lib().b4c_attn_weights_ex(_p(qkv), qkv.stride(0), _p(key_pad), _p(lse), _p(w), B, S, H, dh, dt_code(qkv.dtype),
                                        _st(), ATTN_CAUSAL if causal else 0), 'attn_weights_ex')
    return w


def transpose_add_(dst, src):
    """dst [N, K] += src [K, N]^T (fp32)."""
    K, N = src.shape
    L.check(L.lib().b4c_transpose_add(_p(src), src.stride(0), _p(dst), dst.stride(0), K, N, _st()), 'transpose_add')


def rows_gather_f32(src, idx):
    out = torch.empty(idx.shape[0], src.shape[1], dtype=torch.float32, device=src.device)
    L.check(L.lib().b4c_rows_gather_f32(_p(src), src.stride(0), _p(idx), _p(out), out.stride(0), idx.shape[0], src.shape[1],
                                        _st()), 'rows_gather_f32')
    return out


def rows_scatter_add_f32_(dst, idx, src):
    L.check(L.lib().b4c_rows_scatter_add_f32(_p(src), src.stride(0), _p(idx), _p(dst), dst.stride(0), idx.shape[0],
                                             src.shape[1], _st()), 'rows_scatter_add_f32')


class MHAFn(torch.autograd.Function):
    """MultiHeadAttention.call(v, k, q, mask) in general (transformer.py:137-160): distinct value / key / query inputs
    of one padded length S, key-side padding mask, attention weights on request.  Differentiable in the three inputs
    and all eight parameters.  apply(xq, xk, xv, key_pad, wq, bq, wk, bk, wv, bv, wo, bo, pk_qkv, pk_o, B, S, H, same, want_w
    [, causal])"""

    @staticmethod
    def forward(ctx, xq, xk, xv, key_pad, wq, bq, wk, bk, wv, bv, wo, bo, pk_qkv, pk_o, B, S, H, same, want_w, causal=False):
        T_tok, d = xq.shape
        dh = d // H
        wt_qkv, _, b_qkv = pk_qkv.get(xq.dtype, d, True)
        wt_o, _, b_o = pk_o.get(xq.dtype, d, True)
        if same:
            qkv = gemm_nt(xq, wt_qkv, 3 * d, b_qkv)
        else:
            qkv = torch.empty(T_tok, 3 * d, dtype=xq.dtype, device=xq.device)
            for i, x in enumerate((xq, xk, xv)):
                gemm_nt(x, wt_qkv[i * d:(i + 1) * d], d, b_qkv[i * d:(i + 1) * d], out=qkv[:, i * d:(i + 1) * d])
        ckw = {'causal': True} if causal else {}        # (a bidirectional call is the call it has always been)
        o, lse = attn_fwd(qkv, key_pad, B, S, H, dh, **ckw)
        out = gemm_nt(o, wt_o, d, b_o)
        w = attn_weights(qkv, key_pad, lse, B, S, H, dh, **ckw) if want_w else None
        ctx.save_for_backward(xq, xk, xv, key_pad, qkv, o, lse)
        ctx.pk, ctx.dims, ctx.same, ctx.ckw = (pk_qkv, pk_o), (B, S, H, dh), same, ckw
        ctx.params = (wq, bq, wk, bk, wv, bv, wo, bo)
        if w is None:
            w = torch.empty(0, device=xq.device)
        ctx.mark_non_differentiable(w)
        return out, w

    @staticmethod
    def backward(ctx, dout, _):
        xq, xk, xv, key_pad, qkv, o, lse = ctx.saved_tensors
        pk_qkv, pk_o = ctx.pk
        B, S, H, dh = ctx.dims
        d = H * dh
        _, wc_o, _ = pk_o.get(xq.dtype, d, True)
        _, wc_qkv, _ = pk_qkv.get(xq.dtype, d, True)
        actx, sinks = grad_sinks(*ctx.params)
        gw, gb = sinks[0:8:2], sinks[1:8:2]         # Q, K, V, output projection
        dy = dout.contiguous()
        gemm_tn(o, dy, d, d, into=(gw[3:], gb[3:]))
        d_o = gemm_nt(dy, wc_o, d)
        dqkv = attn_bwd(qkv, key_pad, o, d_o, lse, B, S, H, dh, **ctx.ckw)
        if ctx.same:
            gemm_tn(xq, dqkv, d, 3 * d, into=(gw[:3], gb[:3]))
            gx = (gemm_nt(dqkv, wc_qkv, d), None, None)
        else:
            gx = []
            for i, x in enumerate((xq, xk, xv)):
                g = dqkv[:, i * d:(i + 1) * d]
                gemm_tn(x, g, d, d, into=(gw[i:i + 1], gb[i:i + 1]))
                gx.append(gemm_nt(g, wc_qkv[:, i * d:(i + 1) * d], d))
        _ready(*ctx.params)
        return sink_returns(ctx, tuple(gx) + (None,), actx, sinks)


class TiedPackedLinear(PackedLinear):
    """Compute copies of a projection whose weights are rows off .. off+V of an embedding table (rows, K) fp32,
    vocabulary-major: ``wt`` [Vp][Kp] is a straight copy of those rows, ``wc`` [Kp][Vp] their transpose, ``bias``
    the head's own fp32 [V].  Re-packed with the dense layers (same batched launch: the table slice is handed to
    b4c_pack_weights_batched as a "[V][K] kernel" with the two outputs swapped)."""

    def __init__(self, table, off, V, bias):
        import weakref
        self.table, self.tied_offset, self.bias_p = table, int(off), bias
        self.kernels, self.biases = [table], [bias]
        self.K = int(table.shape[1])
        self.Ns = [int(V)]
        self.N = int(V)
        self.Np = rup8(self.N)
        self._cache = {}
        _pack_registry.append(weakref.ref(self))

    def _descs(self, ent, Kp):
        t = self.table.detach()
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise B4CError('embedding tables must be contiguous float32')
        lz = getattr(self.table, '_b4c_lazy', None)
        if lz is not None:          # row-lazy optimizer: the whole table is about to be read
            lz.sync()
        rows = t[self.tied_offset:self.tied_offset + self.N]
        ent['bias'][:self.N].copy_(self.bias_p.detach())
        # as a Keras kernel [K' = V][N' = K]:  wt'[n'][k'] = src[k'][n'] is our wc [K][V],  wc'[k'][n'] is our wt [V][K]
        return [L.PackDesc(rows.data_ptr(), None, ent['wc'].data_ptr() if ent['wc'] is not None else None,
                           ent['wt'].data_ptr(), None, self.N, self.K, self.Np, Kp, 0, 0)]


class TiedLogitsFn(torch.autograd.Function):
    """logits [R, Vp] = h . E[off : off + V]^T + bias for the tied-weight head (materialised route)."""

    @staticmethod
    def forward(ctx, h, table, bias, pack, out_fp32):
        h = h.contiguous()
        wt, _, b = pack.get(h.dtype, h.shape[1], True)
        ctx.save_for_backward(h)
        ctx.pack, ctx.params = pack, (table, bias)
        odt = torch.float32 if out_fp32 else h.dtype
        return gemm_nt(h, wt, pack.Np, b, out_dtype=odt, out=empty_rows(h.shape[0], pack.Np, odt, h.device))

    @staticmethod
    def backward(ctx, g):
        (h,) = ctx.saved_tensors
        pack = ctx.pack
        table, bias = ctx.params
        g = _rows_ok(g, h.dtype)
        _, wc, _ = pack.get(h.dtype, h.shape[1], True)
        dWt, db = gemm_tn(h, g, pack.K, pack.N)                 # [K, V] fp32, [V]
        dh = gemm_nt(g, wc, h.shape[1])
        off = pack.tied_offset
        _tied_table_steps_whole(table)
        actx, (dtab, dbias) = grad_sinks(table, bias)
        transpose_add_(dtab[off:off + pack.N], dWt)
        dbias += db
        _ready(bias)
        return sink_returns(ctx, (dh,), actx, (dtab, dbias))


# --------------------------------------------------------------------------------------
# sampled-softmax head (config 5; no reference counterpart)
# --------------------------------------------------------------------------------------
def log_uniform_sample(seed, n, range_max, device):
    """n ids (int64) from the log-uniform sampler over [0, range_max) with replacement, and log Q(id) (fp32)."""
    ids = torch.empty(n, dtype=torch.int64, device=device)
    logq = torch.empty(n, dtype=torch.float32, device=device)
    L.check(L.lib().b4c_log_uniform_sample(int(seed) & 0xFFFFFFFFFFFFFFFF, n, range_max, _p(ids), _p(logq), _st()),
            'log_uniform_sample')
    return ids, logq


def row_dot(a, b):
    out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    L.check(L.lib().b4c_row_dot(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), a.shape[0], a.shape[1], dt_code(a.dtype),
                                _st()), 'row_dot')
    return out


def scatter_add_1d_(dst, idx, src):
    L.check(L.lib().b4c_scatter_add_1d(_p(src), _p(idx), _p(dst), idx.shape[0], _st()), 'scatter_add_1d')


def row_scale_f32(src, scale):
    out = torch.empty(src.shape[0], src.shape[1], dtype=torch.float32, device=src.device)
    L.check(L.lib().b4c_row_scale_f32(_p(src), src.stride(0), _p(scale), _p(out), out.stride(0), src.shape[0], src.shape[1],
                                      dt_code(src.dtype), _st()), 'row_scale_f32')
    return out


class SampledCEFn(torch.autograd.Function):
    """Sampled-softmax masked-item loss (tf.nn.sampled_softmax_loss semantics: shared log-uniform negatives, logQ
    correction, accidental hits removed), mean over valid rows.  The vocabulary-major projection table (V, K) is only
    touched at the sampled and the label rows: its gradient is row-sparse.
    apply(h [R, K], table (V, K) fp32, bias (V,) fp32, labels_i32 [R], samples int64 [Ns], logq fp32 [Ns], unit_grad)"""

    @staticmethod
    def forward(ctx, h, table, bias, labels_i32, samples, logq, unit_grad):
        h = h.contiguous()
        V, Kd = table.shape
        Ns = samples.shape[0]
        valid_m = (labels_i32 >= 0) & (labels_i32 < V)
        valid = valid_m.sum().to(torch.float32)
        scale = torch.where(valid > 0, 1.0 / valid.clamp(min=1.0), torch.zeros_like(valid)).reshape(1)
        tab = table.detach()
        idx_y = torch.where(valid_m, labels_i32, torch.full_like(labels_i32, -1)).to(torch.int64)
        lz = getattr(table, '_b4c_lazy', None)
        if lz is not None:          # row-lazy optimizer: the sampled and the label rows are brought up to date before they are read
            lz.catch_up(samples, note=ctx.needs_input_grad[1])
            lz.catch_up(idx_y, note=ctx.needs_input_grad[1])
        Ws = rows_gather_f32(tab, samples).to(h.dtype)                               # [Ns, K]
        bs = (bias.detach()[samples] - logq).contiguous()
        Z = gemm_nt(h, Ws, Ns, bs)                                                   # negatives' logits, bias - logQ folded in
        Wy = rows_gather_f32(tab, idx_y).to(h.dtype)                                 # [R, K], zero rows where ignored
        ztrue = row_dot(h, Wy) + bias.detach()[idx_y.clamp(min=0)]
        item = torch.empty(h.shape[0], dtype=torch.float32, device=h.device)
        dtrue = torch.empty(h.shape[0], dtype=torch.float32, device=h.device)
        if h.shape[0]:
            L.check(L.lib().b4c_sampled_ce_fwd_bwd(_p(Z), Z.stride(0), _p(ztrue), _p(samples), _p(labels_i32), V, _p(item),
                                                   _p(dtrue), _p(scale), h.shape[0], Ns, dt_code(Z.dtype), _st()),
                    'sampled_ce_fwd_bwd')
        ctx.save_for_backward(h, Z, dtrue, Ws, Wy, samples, idx_y)
        ctx.params, ctx.unit_grad = (table, bias), unit_grad
        return item.sum() * scale[0]

    @staticmethod
    def backward(ctx, g):
        h, dZ, dtrue, Ws, Wy, samples, idx_y = ctx.saved_tensors
        table, bias = ctx.params
        Kd = h.shape[1]
        if not ctx.unit_grad:
            dZ = dZ * g.to(dZ.dtype)
            dtrue = dtrue * g.to(torch.float32)
        dh = gemm_nt(dZ, Ws.t().contiguous(), Kd)
        dh = torch.addcmul(dh, dtrue.to(dh.dtype)[:, None], Wy)
        dWT, dbs = gemm_tn(h, dZ, Kd, dZ.shape[1])                  # [K, Ns] = h^T dZ, [Ns] = column sums of dZ
        dWs = torch.zeros(dZ.shape[1], Kd, dtype=torch.float32, device=h.device)
        transpose_add_(dWs, dWT)
        dWy = row_scale_f32(h, dtrue)
        actx, (tg, bg) = grad_sinks(table, bias)
        rows_scatter_add_f32_(tg, samples, dWs)
        rows_scatter_add_f32_(tg, idx_y, dWy)
        scatter_add_1d_(bg, samples, dbs.contiguous())
        scatter_add_1d_(bg, idx_y, dtrue.contiguous())
        _ready(table, bias)
        return sink_returns(ctx, (dh,), actx, (tg, bg))


class CandidateLossFn(torch.autograd.Function):
    """Sampled-negative masked-item loss over each row's own candidate list, target in column 0 (include/b4c.h):
    'bce' (SASRec; its target term times beta: gBCE), 'softmax' (list-wise) or 'bpr', mean over the
    rows with a valid target.  The table -- vocabulary-major projection (row_off 0) or tied item embedding (row_off = its id
    offset) -- is read and receives gradient at the listed rows only.
    apply(h [R, K], table (rows, K) fp32, bias (V,) fp32, cand int32 [R, C], row_off, kind, unit_grad[, shared_table[, beta[, corr[,
          correct_target]]]])
    shared_table: the table is the embedding layer's too, whose backward runs last and announces its gradient.  beta, corr,
    correct_target: candidate_loss_fwd_ex's; corr is data (fp32 [V], no gradient).  With all three at their defaults and kind 'bce'
    or 'softmax' the forward is candidate_loss_fwd -- the same kernel, the same bits."""

    @staticmethod
    def forward(ctx, h, table, bias, cand, row_off, kind, unit_grad, shared_table=False, beta=1.0, corr=None, correct_target=False):
        h = h.contiguous()
        V = bias.shape[0]
        present = (cand >= 0) & (cand < V)
        valid = present[:, 0].sum().to(torch.float32)
        scale = torch.where(valid > 0, 1.0 / valid.clamp(min=1.0), torch.zeros_like(valid)).reshape(1)
        lz = getattr(table, '_b4c_lazy', None)
        if lz is not None:          # row-lazy optimizer: the listed rows are brought up to date before they are read
            lz.catch_up(torch.where(present, cand + int(row_off), torch.full_like(cand, -1)), note=ctx.needs_input_grad[1])
        if kind in CAND_LOSS_KINDS and beta == 1.0 and corr is None and not correct_target:
            item, g, _ = candidate_loss_fwd(h, table.detach(), bias.detach(), cand, V, kind, row_off)
        else:
            item, g, _ = candidate_loss_fwd_ex(h, table.detach(), bias.detach(), cand, V, kind, row_off, False, beta,
                                               None if corr is None else corr.detach(), correct_target)
        ctx.save_for_backward(h, g, cand, scale)
        ctx.params, ctx.row_off, ctx.unit_grad, ctx.shared_table = (table, bias), int(row_off), unit_grad, bool(shared_table)
        return item.sum() * scale[0]

    @staticmethod
    def backward(ctx, gout):
        h, g, cand, scale = ctx.saved_tensors
        table, bias = ctx.params
        gscale = scale if ctx.unit_grad else scale * gout.to(torch.float32)
        actx, (tg, bg) = grad_sinks(table, bias)
        dh = candidate_loss_bwd(h, table.detach(), cand, g, gscale.contiguous(), bias.shape[0], tg, bg, ctx.row_off)
        _ready(*((bias,) if ctx.shared_table else (table, bias)))
        return sink_returns(ctx, (dh,), actx, (tg, bg))


class InfoNCEFn(torch.autograd.Function):
    """In-batch contrastive loss (NT-Xent / InfoNCE; include/b4c.h): the mean of nce_fwd's item_loss over the live rows -- rows
    whose pos names another row of the batch.  apply(z [N, K], pos int32 [N], group int32 [N] or None, temperature, similarity) ->
    scalar.  The count of live rows and gscale = 1 / max(count, 1) are formed on the device: no read-back."""

    @staticmethod
    def forward(ctx, z, pos, group, temperature=1.0, similarity='dot'):
        z = z.contiguous()
        N = z.shape[0]
        item, lse, rnorm = nce_fwd(z, pos, group, temperature, similarity)
        idx = torch.arange(N, dtype=torch.int32, device=z.device)
        live = ((pos >= 0) & (pos < N) & (pos != idx)).sum().to(torch.float32)
        scale = (1.0 / live.clamp(min=1.0)).reshape(1)
        ctx.save_for_backward(z, pos, lse, scale, *(() if rnorm is None else (rnorm,)))
        ctx.group, ctx.temperature, ctx.similarity = group, temperature, similarity
        return item.sum() * scale[0]

    @staticmethod
    def backward(ctx, gout):
        z, pos, lse, scale = ctx.saved_tensors[:4]
        rnorm = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        gscale = (scale * gout.to(torch.float32)).contiguous()
        dz = nce_bwd(z, pos, ctx.group, ctx.temperature, ctx.similarity, rnorm, lse, gscale)
        return dz, None, None, None, None
