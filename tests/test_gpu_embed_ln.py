"""The embedding stage with LayerNorm (b4c_embed_ln_fwd / _bwd) and the plain LayerNorm (b4c_layernorm_fwd / _bwd) through
their ops wrappers.  NO REFERENCE ORACLE: extensions of the BERT4Rec paper -- the float64 restatement is
tests/paper_model_ref.py.  Shapes: the smallest that reach every branch of the row kernels (one lane per row, idle lanes inside a
16-lane group, whole 16- and 32-lane groups, a second pass), B = 3, S = 7 and T = 1.

Bounds.  Forward: fp32 1e-4 absolute (the project's activation bar); bf16 2^-8 |value| + 1e-4 (one rounding of an fp32 result,
doubled).  stats: mean and rstd 1e-5 relative, each element; the tables, learned positions and x carry an offset of the order of
their spread, so that a row's mean is of the order of its terms (a sum that cancels to nothing has no relative accuracy in any
arithmetic) while rstd stays of order 1.  Backward: 2e-4 relative L2 in fp32 for dpre, dgamma, dbeta, the
tables' gradients and dP; bf16 (dout holds bf16-representable values): dpre 2^-8 relative L2, dgamma / dbeta 1e-3; the tables'
gradients and dP there are held against float64 sums of the DEVICE's own bf16 dpre (exact inputs of the existing kernels, fp32
accumulation: 2e-4), which checks what this stage hands those kernels -- ids, scale, no second dropout."""
import functools

import numpy as np
import pytest
import torch

import paper_model_ref as pm

pytestmark = pytest.mark.gpu

SEED, SCALE, G = 1234, 1.25, 2          # G: guard rows (and 8 guard columns) around every output
# name -> (feature widths, combine)
CASES = {'d8': ((8,), 'concat'), 'cat48+24': ((48, 24), 'concat'), 'd128': ((128,), 'concat'), 'sum64+64': ((64, 64), 'sum'),
         'd256': ((256,), 'concat'), 'd520': ((520,), 'concat')}
ROWS = 11                               # table rows: ids run from -2 to ROWS + 3


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops as o
    return o


def _ids(B, S, n_feat, g):
    """first feature: [CLS]-like 1 first, the closing 3 at S - 1, pads (0) BEFORE it, an id past the table and a negative one;
    further features: anything from -2 to ROWS + 3, zeros included"""
    first = torch.randint(4, ROWS, (B, S), generator=g)
    first[:, 0], first[:, S - 1] = 1, 3
    if S > 4:
        first[0, S - 3:S - 1] = 0
        first[B - 1, 2:S - 1] = 0
        first[0, 1], first[B - 1, 1] = ROWS + 3, -2
    return [first] + [torch.randint(-2, ROWS + 4, (B, S), generator=g) for _ in range(n_feat - 1)]


@functools.lru_cache(maxsize=None)
def _case(name, layout, learned, rate, B=3, S=7):
    """inputs and the float64 results of one configuration, computed once and shared by the fp32 and the bf16 test"""
    from bert4clickpath_amd import ops
    widths, combine = CASES[name]
    d = widths[0] if combine == 'sum' else sum(widths)
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 31 * B + (7 if learned else 0))
    ids = _ids(B, S, len(widths), g)
    tables = [torch.randn(ROWS, w, generator=g) * 0.5 + 0.75 for w in widths]
    pe = torch.randn(S + 2, d, generator=g) * 0.5 + 0.5 if learned else pm.tr.positional_encoding(S + 2, d)
    gamma, beta = 1 + 0.3 * torch.randn(d, generator=g), 0.2 * torch.randn(d, generator=g)
    src = torch.arange(B * S) if layout == 'dense' else torch.nonzero(ids[0].reshape(-1) != 0)[:, 0]
    T = int(src.numel())
    dout = torch.randn(T, d, generator=g).bfloat16().float()
    keep = torch.from_numpy(np.asarray(ops.keep_mask(SEED, T * d, rate)).reshape(T, d)) if rate > 0 else None
    D = [t.double() for t in tables]
    pre = pm.embed_pre(ids, D, pe.double(), SCALE, combine).reshape(B * S, d)[src]
    mean, rstd = pm.ln_stats(pre)
    out = pm.tr.dropout(pm.tr.layer_norm(pre, gamma.double(), beta.double(), pm.EPS), rate, keep)
    dpre, dgamma, dbeta = pm.ln_backward(dout.double(), pre, gamma.double(), keep, rate)
    return dict(B=B, S=S, d=d, T=T, combine=combine, ids=ids, tables=tables, pe=pe, gamma=gamma, beta=beta, src=src, dout=dout,
                keep=keep, pre=pre, mean=mean[:, 0], rstd=rstd[:, 0], out=out, dpre=dpre, dgamma=dgamma, dbeta=dbeta)


def _table_grads(c, dpre):
    """float64: what the plain stage's backward makes of dout = dpre at rate 0 -> ([dtable_f], dP [S, d])"""
    B, S, d = c['B'], c['S'], c['d']
    outs, col = [], 0
    for i, t in zip(c['ids'], c['tables']):
        w = t.shape[1]
        gt = torch.zeros(t.shape, dtype=torch.float64)
        gt.index_add_(0, i.reshape(-1)[c['src']].clamp(0, t.shape[0] - 1), SCALE * dpre[:, col:col + w])
        outs.append(gt)
        col += 0 if c['combine'] == 'sum' else w
    dP = torch.zeros(S, d, dtype=torch.float64)
    dP.index_add_(0, c['src'] % S, dpre)
    return outs, dP


def _packed(ops, c):
    if c['T'] == c['B'] * c['S']:
        return None
    B, S, T = c['B'], c['S'], c['T']
    real = c['ids'][0] != 0
    cu = torch.cat([torch.zeros(1, dtype=torch.int64), real.sum(1).cumsum(0)]).to(torch.int32)
    packed_of = torch.full((B * S,), -1, dtype=torch.int32)
    packed_of[c['src']] = torch.arange(T, dtype=torch.int32)
    return ops.Packed(cu.cuda(), c['src'].to(torch.int32).cuda(), packed_of.cuda(), B, S, T, int(real.sum(1).max()))


def _guarded(T, n, dtype):
    """(buffer filled with 7, its [T, n] inner view): G guard rows above and below, 8 guard columns to the right"""
    buf = torch.full((T + 2 * G, n + 8), 7.0, dtype=dtype, device='cuda')
    return buf, buf[G:G + T, :n]


def _guards_intact(buf, T, n):
    ok = torch.ones_like(buf, dtype=torch.bool)
    ok[G:G + T, :n] = False
    return bool((buf[ok] == 7.0).all())


def _rel(got, want):
    return float((got.double().cpu() - want).norm() / want.norm())


def _run(ops, c, dtype, rate):
    """forward and backward of one configuration, twice, into guarded buffers -> dict of device results (second launch checked)"""
    dev = lambda ts: [t.cuda() for t in ts]
    ids, tables, pe, gamma, beta = dev(c['ids']), dev(c['tables']), c['pe'].cuda(), c['gamma'].cuda(), c['beta'].cuda()
    packed = _packed(ops, c)
    T, d = c['T'], c['d']
    runs = []
    for _ in range(2):
        obuf, out = _guarded(T, d, dtype)
        sbuf = torch.full((T + 2 * G, 2), 7.0, device='cuda')
        pbuf, dpre = _guarded(T, d, dtype)
        _, key_pad, stats = ops.embed_ln_fwd(ids, tables, pe, SCALE, gamma, beta, rate, SEED, dtype, packed, c['combine'], out=out,
                                             stats=sbuf[G:G + T])
        dgamma, dbeta = torch.full((d,), 0.5, device='cuda'), torch.full((d,), -0.25, device='cuda')      # sinks: ADDED to
        ops.embed_ln_bwd(ids, tables, pe, SCALE, gamma, stats, c['dout'].to(dtype).cuda(), rate, SEED, packed, c['combine'],
                         into=(dgamma, dbeta), dpre=dpre)
        assert _guards_intact(obuf, T, d) and _guards_intact(pbuf, T, d)
        assert bool((sbuf[:G] == 7.0).all()) and bool((sbuf[G + T:] == 7.0).all())
        runs.append(dict(out=out.clone(), key_pad=key_pad, stats=stats.clone(), dpre=dpre.clone(), dgamma=dgamma - 0.5, dbeta=dbeta + 0.25))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), 'second launch: %s differs' % k
    r = runs[0]
    # the existing kernels on dpre: packed ids [1, T] as EmbedFn's backward takes them
    pk_ids = [i.reshape(-1)[c['src'].cuda()].reshape(1, T).contiguous() for i in ids]
    r['dtables'] = ops.embed_concat_pe_bwd(pk_ids, tables, r['dpre'].reshape(1, T, d).contiguous(), SCALE, 0.0, 0)
    B, S = c['B'], c['S']
    r['dP'] = ops.pos_table_bwd(r['dpre'], ops.dense_cu(B, S, 'cuda') if packed is None else None, B, S, 0.0, 0,
                                torch.zeros(S, d, device='cuda'), row_of=packed.packed_of if packed is not None else None)
    return r


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('name', list(CASES))
def test_embed_ln_against_float64(ops, name, dtype):
    worst = {}
    for layout in ('dense', 'packed'):
        for learned in (False, True):
            for rate in (0.0, 0.25):
                c = _case(name, layout, learned, rate)
                assert (c['T'] < c['B'] * c['S']) == (layout == 'packed')
                r = _run(ops, c, dtype, rate)
                tag = (layout, 'learned' if learned else 'sinusoidal', rate)
                # ---- forward
                out, want = r['out'].double().cpu(), c['out']
                err = (out - want).abs()
                bound = 1e-4 if dtype == torch.float32 else 2.0 ** -8 * want.abs() + 1e-4
                worst['out'] = max(worst.get('out', 0.0), float(err.max()))
                assert bool((err <= bound).all()), (tag, float(err.max()))
                if rate > 0:
                    assert bool((out[~c['keep']] == 0).all()) and 0 < int((~c['keep']).sum()) < c['keep'].numel() // 2
                assert torch.equal(r['key_pad'].reshape(-1).cpu(), (c['ids'][0].reshape(-1)[c['src']] == 0).to(torch.uint8))
                mean, rstd = r['stats'][:, 0].double().cpu(), r['stats'][:, 1].double().cpu()
                assert bool(((mean - c['mean']).abs() <= 1e-5 * c['mean'].abs()).all()) and float(c['mean'].abs().min()) > 0.2, tag
                assert bool(((rstd - c['rstd']).abs() <= 1e-5 * c['rstd']).all()) and 0.3 < float(c['rstd'].median()) < 3, tag
                # ---- backward
                e = {k: _rel(r[k], c[k]) for k in ('dpre', 'dgamma', 'dbeta')}
                fp32 = dtype == torch.float32
                assert e['dpre'] < (2e-4 if fp32 else 2.0 ** -8), (tag, e)
                assert e['dgamma'] < (2e-4 if fp32 else 1e-3) and e['dbeta'] < (2e-4 if fp32 else 1e-3), (tag, e)
                want_t, want_P = _table_grads(c, c['dpre'] if fp32 else r['dpre'].double().cpu())
                for f, (gt, wt) in enumerate(zip(r['dtables'], want_t)):
                    e['dtable%d' % f] = _rel(gt, wt)
                    assert e['dtable%d' % f] < 2e-4, (tag, e)
                if learned:
                    e['dP'] = _rel(r['dP'], want_P)
                    assert e['dP'] < 2e-4, (tag, e)
                for k, v in e.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print(name, dtype, ' '.join('%s %.2e' % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_one_token(ops, dtype):
    """T = 1: one row, one workgroup, every other row group of the workgroup idle"""
    c = _case('d128', 'dense', True, 0.25, B=1, S=1)
    assert c['T'] == 1
    r = _run(ops, c, dtype, 0.25)
    fp32 = dtype == torch.float32
    err = (r['out'].double().cpu() - c['out']).abs()
    assert bool((err <= (1e-4 if fp32 else 2.0 ** -8 * c['out'].abs() + 1e-4)).all())
    assert _rel(r['dpre'], c['dpre']) < (2e-4 if fp32 else 2.0 ** -8)
    assert _rel(r['dgamma'], c['dgamma']) < (2e-4 if fp32 else 1e-3) and _rel(r['dbeta'], c['dbeta']) < (2e-4 if fp32 else 1e-3)


def test_refusals(ops):
    from bert4clickpath_amd._lib import B4CError
    c = _case('d128', 'dense', False, 0.0)
    ids, tables = [t.cuda() for t in c['ids']], [t.cuda() for t in c['tables']]
    pe, gamma, beta = c['pe'].cuda(), c['gamma'].cuda(), c['beta'].cuda()
    out, _, stats = ops.embed_ln_fwd(ids, tables, pe, SCALE, gamma, beta, 0.0, 0, torch.float32)
    dout = c['dout'].cuda()
    need = ops.L.lib().b4c_embed_ln_bwd_workspace_bytes(c['T'], c['d'])
    assert need > 0 and need == ops.L.lib().b4c_layernorm_bwd_workspace_bytes(c['T'], c['d'])
    small = torch.empty(need - 1, dtype=torch.uint8, device='cuda')
    with pytest.raises(B4CError, match='workspace too small'):
        ops.embed_ln_bwd(ids, tables, pe, SCALE, gamma, stats, dout, 0.0, 0, workspace=small)
    ops.embed_ln_bwd(ids, tables, pe, SCALE, gamma, stats, dout, 0.0, 0, workspace=torch.empty(need, dtype=torch.uint8, device='cuda'))
    x = out.reshape(-1, c['d'])
    with pytest.raises(B4CError, match='workspace too small'):
        ops.layernorm_bwd(dout, x, stats, gamma, workspace=small)
    with pytest.raises(B4CError):          # a row wider than the row kernels hold
        wide = [torch.zeros(ROWS, 1032, device='cuda')]
        ops.embed_ln_fwd(ids[:1], wide, torch.zeros(c['S'], 1032, device='cuda'), 1.0, torch.ones(1032, device='cuda'),
                         torch.zeros(1032, device='cuda'), 0.0, 0, torch.float32)
    with pytest.raises(B4CError):          # a positional table shorter than the sequences
        ops.embed_ln_fwd(ids, tables, pe[:c['S'] - 1].contiguous(), SCALE, gamma, beta, 0.0, 0, torch.float32)
    with pytest.raises(B4CError):
        ops.embed_ln_fwd(ids, tables, pe, SCALE, gamma[:-8].contiguous(), beta, 0.0, 0, torch.float32)


# ---- plain LayerNorm ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ln_case(rows, d):
    g = torch.Generator().manual_seed(rows * 1000 + d)
    x = (torch.randn(rows, d, generator=g) * 0.5 + 0.75).bfloat16().float()          # representable in both dtypes
    u = torch.randn(rows, d, generator=g).bfloat16().float()                          # a pre-activation for the gate
    gamma, beta = 1 + 0.3 * torch.randn(d, generator=g), 0.2 * torch.randn(d, generator=g)
    dout = torch.randn(rows, d, generator=g).bfloat16().float()
    X = x.double()
    mean, rstd = pm.ln_stats(X)
    dx, dgamma, dbeta = pm.ln_backward(dout.double(), X, gamma.double())
    return dict(x=x, u=u, gamma=gamma, beta=beta, dout=dout, out=pm.tr.layer_norm(X, gamma.double(), beta.double(), pm.EPS),
                mean=mean[:, 0], rstd=rstd[:, 0], dx=dx, dgamma=dgamma, dbeta=dbeta)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('d', [64, 72, 256])
@pytest.mark.parametrize('rows', [1, 37])
def test_layernorm_against_float64(ops, rows, d, dtype):
    c = _ln_case(rows, d)
    fp32 = dtype == torch.float32
    x, gamma, beta, dout = c['x'].to(dtype).cuda(), c['gamma'].cuda(), c['beta'].cuda(), c['dout'].to(dtype).cuda()
    runs = []
    for _ in range(2):
        obuf = torch.full((rows + 2 * G, d), 7.0, dtype=dtype, device='cuda')
        sbuf = torch.full((rows + 2 * G, 2), 7.0, device='cuda')
        dbuf = torch.full((rows + 2 * G, d), 7.0, dtype=dtype, device='cuda')
        out, stats = ops.layernorm_fwd(x, gamma, beta, out=obuf[G:G + rows], stats=sbuf[G:G + rows])
        dgamma, dbeta = torch.full((d,), 0.5, device='cuda'), torch.full((d,), -0.25, device='cuda')
        dx, _, _ = ops.layernorm_bwd(dout, x, stats, gamma, into=(dgamma, dbeta), dx=dbuf[G:G + rows])
        for buf in (obuf, sbuf, dbuf):
            assert bool((buf[:G] == 7.0).all()) and bool((buf[G + rows:] == 7.0).all())
        runs.append((out.clone(), stats.clone(), dx.clone(), dgamma - 0.5, dbeta + 0.25))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    out, stats, dx, dgamma, dbeta = runs[0]
    err = (out.double().cpu() - c['out']).abs()
    assert bool((err <= (1e-4 if fp32 else 2.0 ** -8 * c['out'].abs() + 1e-4)).all()), float(err.max())
    assert bool(((stats[:, 0].double().cpu() - c['mean']).abs() <= 1e-5 * c['mean'].abs()).all())
    assert bool(((stats[:, 1].double().cpu() - c['rstd']).abs() <= 1e-5 * c['rstd']).all())
    assert _rel(dx, c['dx']) < (2e-4 if fp32 else 2.0 ** -8)
    assert _rel(dgamma, c['dgamma']) < (2e-4 if fp32 else 1e-3) and _rel(dbeta, c['dbeta']) < (2e-4 if fp32 else 1e-3)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('act', ['relu', 'gelu', 'gelu_tanh'])
def test_layernorm_backward_gate(ops, act, dtype):
    """dx * act'(gate) as the head's transform needs it: the same dx, gated by the float64 derivative (pitched gate view)"""
    rows, d = 37, 72
    c = _ln_case(rows, d)
    fp32 = dtype == torch.float32
    x, gamma, dout = c['x'].to(dtype).cuda(), c['gamma'].cuda(), c['dout'].to(dtype).cuda()
    _, stats = ops.layernorm_fwd(x, gamma, c['beta'].cuda())
    gbuf = torch.zeros(rows, d + 8, dtype=dtype, device='cuda')
    gbuf[:, :d] = c['u'].to(dtype).cuda()
    dx, dgamma, dbeta = ops.layernorm_bwd(dout, x, stats, gamma, gate=gbuf[:, :d], gate_act=ops.ffn_act_code(act))
    want = c['dx'] * pm.pr.act_grad(act, c['u'].double())
    assert _rel(dx, want) < (2e-4 if fp32 else 2.0 ** -8)
    assert _rel(dgamma, c['dgamma']) < (2e-4 if fp32 else 1e-3) and _rel(dbeta, c['dbeta']) < (2e-4 if fp32 else 1e-3)
