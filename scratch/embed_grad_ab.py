"""python scratch/embed_grad_ab.py OTHER_LIBB4C_HIP_SO [OUT.json]
A/B of b4c_sort_ids, b4c_embed_concat_pe_bwd_sorted_ws and b4c_pack_weights_batched: another build's library ("old", e.g. the parent
commit's) against this tree's ("new"), both loaded into one process: same inputs, outputs compared bit for bit, times by device
events (median and minimum of `reps` launches).  DESIGN.md section 5 / profiles/embed_grad_ab.txt."""
import ctypes, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4clickpath_amd import _lib as LB, ops

new = LB.lib()
old = ctypes.CDLL(os.path.abspath(sys.argv[1]))
NAMES = ['b4c_sort_ids', 'b4c_sort_ids_workspace_bytes', 'b4c_embed_concat_pe_bwd_sorted_ws', 'b4c_embed_concat_pe_bwd_sorted',
         'b4c_embed_concat_pe_bwd_sorted_workspace_bytes', 'b4c_pack_weights_batched', 'b4c_last_error']
for nme in NAMES:
    getattr(old, nme).restype = getattr(new, nme).restype
    getattr(old, nme).argtypes = getattr(new, nme).argtypes
st = torch.cuda.current_stream().cuda_stream
dev = 'cuda'
res = {}


def timed(fn, reps=30, flush=None):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        if flush is not None:
            flush()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000)
    ts.sort()
    return round(ts[len(ts) // 2], 1), round(ts[0], 1)


def zipf_ids(n, rows, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, generator=g)
    return (torch.exp(u * np.log(rows + 1.0)) - 1).long().clamp_(0, rows - 1)


# ---- sort
for n, rows in ((455000, 50003), (41000, 50001), (1200000, 50003)):
    ids = zipf_ids(n, rows, n).to(dev)
    out = {}
    for tag, lib in (('old', old), ('new', new)):
        need = int(lib.b4c_sort_ids_workspace_bytes(n, rows))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        order = torch.empty(n, dtype=torch.int32, device=dev)
        fn = lambda: lib.b4c_sort_ids(ids.data_ptr(), n, rows, order.data_ptr(), ws.data_ptr(), need, st)
        assert fn() == 0, lib.b4c_last_error()
        res['sort_%d_%s_us(med,min)' % (n, tag)] = timed(fn)
        out[tag] = order.clone()
    want = torch.sort(ids, stable=True)[1].int()
    res['sort_%d_equal' % n] = bool(torch.equal(out['old'], out['new']) and torch.equal(out['new'], want))
    print(json.dumps({k: v for k, v in res.items() if k.startswith('sort_%d' % n)}), flush=True)

# ---- scatter: the bench's shape (455 k packed tokens, one feature of 128, 50 k rows, bf16, rate 0.1)
T, d, rows = 455000, 128, 50003
ids = zipf_ids(T, rows, 5).to(dev)
order = torch.sort(ids, stable=True)[1].int()
for dtype in (torch.bfloat16, torch.float32):
    dout = torch.randn(T, d, device=dev).to(dtype)
    for rate in (0.1, 0.0):
        out = {}
        for tag, lib in (('old', old), ('new', new)):
            dims = (ctypes.c_int * 1)(d)
            ra = (ctypes.c_int64 * 1)(rows)
            need = int(lib.b4c_embed_concat_pe_bwd_sorted_workspace_bytes(1, dims, 1, T))
            ws = torch.zeros(need, dtype=torch.uint8, device=dev)
            tab = torch.zeros(rows, d, device=dev)
            ia, oa, ta = (ctypes.c_void_p * 1)(ids.data_ptr()), (ctypes.c_void_p * 1)(order.data_ptr()), (ctypes.c_void_p * 1)(tab.data_ptr())
            fn = lambda: lib.b4c_embed_concat_pe_bwd_sorted_ws(1, ia, oa, ta, dims, ra, 11.3, dout.data_ptr(), d, 1, T, d, rate, 12345,
                                                               ws.data_ptr(), need, ops.dt_code(dtype), st)
            assert fn() == 0, lib.b4c_last_error()
            out[tag] = tab.clone()
            fn(); fn()
            out[tag + '3'] = tab.clone()
            res['scatter_%s_%g_%s_us(med,min)' % (str(dtype)[6:], rate, tag)] = timed(fn, flush=lambda: tab.zero_())
        k = 'scatter_%s_%g' % (str(dtype)[6:], rate)
        res[k + '_equal'] = bool(torch.equal(out['old'], out['new']) and torch.equal(out['old3'], out['new3']))
        print(json.dumps({kk: v for kk, v in res.items() if kk.startswith(k)}), flush=True)

# ---- pack: the vocabulary projection [128][50000] alone, warm and with the source pushed out of the caches
K, N = 128, 50000
w = torch.randn(K, N, device=dev)
bias = torch.randn(N, device=dev)
junk = torch.empty(768 << 20, dtype=torch.uint8, device=dev)
for tag, lib in (('old', old), ('new', new)):
    wt = torch.zeros(N, K, dtype=torch.bfloat16, device=dev)
    wc = torch.zeros(K, N, dtype=torch.bfloat16, device=dev)
    bd = torch.zeros(N, device=dev)
    desc = LB.PackDesc(w.data_ptr(), bias.data_ptr(), wt.data_ptr(), wc.data_ptr(), bd.data_ptr(), K, N, K, N, 0, 0)
    dd = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(dev)
    tiles = ((K + 63) // 64) * ((N + 63) // 64)
    fn = lambda: lib.b4c_pack_weights_batched(dd.data_ptr(), 1, tiles, ops.dt_code(torch.bfloat16), st)
    assert fn() == 0
    res['pack_%s_equal' % tag] = bool(torch.equal(wt, w.t().contiguous().to(torch.bfloat16)) and torch.equal(wc, w.to(torch.bfloat16)) and torch.equal(bd, bias))
    res['pack_warm_%s_us(med,min)' % tag] = timed(fn)
    res['pack_cold_%s_us(med,min)' % tag] = timed(fn, flush=lambda: junk.fill_(1))
    # one output at a time
    for what, (a_, b_) in (('wt_only', (wt, None)), ('wc_only', (None, wc))):
        desc = LB.PackDesc(w.data_ptr(), bias.data_ptr(), a_.data_ptr() if a_ is not None else None, b_.data_ptr() if b_ is not None else None,
                           bd.data_ptr(), K, N, K, N, 0, 0)
        d2 = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(dev)
        f2 = lambda: lib.b4c_pack_weights_batched(d2.data_ptr(), 1, tiles, ops.dt_code(torch.bfloat16), st)
        res['pack_%s_%s_us(med,min)' % (what, tag)] = timed(f2)
print(json.dumps({k: v for k, v in res.items() if k.startswith('pack')}), flush=True)
if len(sys.argv) > 2:
    json.dump(res, open(sys.argv[2], 'w'), indent=1)
