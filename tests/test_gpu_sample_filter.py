"""afhip_sample_filter on the GPU against the float64 oracle of tests/sample_ref.py: kept sets, processed rows, draws, the distribution
over a u grid, edge cases, agreement with afhip_sample_topk, and bit-determinism (two launches, hipGraph replay)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MODES = {  # name: (penalty, temperature, top_k, exact_k, top_p)
    "hf_all": (1.05, 0.7, 20, False, 0.8),
    "top_p": (1.0, 1.0, 0, False, 0.95),
    "exact_k": (1.0, 0.9, 1000, True, 1.0),
    "hf_k_big": (1.0, 1.0, 5000, False, 1.0),
    "pen_only": (1.3, 1.0, 0, False, 1.0),
    "k_then_p": (1.0, 1.2, 300, True, 0.6),
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")


def _rows(rows, V, seed, peak=0.0):
    """randn rows; peak > 0 lifts 64 random ids of each row by `peak`, so that they carry nearly all the mass and the cumulative
    masses near a top-p boundary are far apart (a flat 152k-id row has ~1e-5 per id: no p would be 1e-5 away from every step)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, V, generator=g) * 2.5).float()
    if peak:
        for r in range(rows):
            x[r, torch.randperm(V, generator=g)[:64]] += peak
    return x


def _ids(rows, V, seed, n=48):
    g = torch.Generator().manual_seed(seed + 1)
    return torch.randint(0, V, (rows, n), generator=g, dtype=torch.int32)


def _run(lg, u=None, ids=None, n_ids=None, scores=True, **kw):
    from audio_intelligence_amd import ops
    d = lg.to(DEV).contiguous()
    sc = torch.full(d.shape, 7.0, device=DEV) if scores else None
    tok = ops.sample_filter(d, u=None if u is None else u.to(DEV), penalty_ids=None if ids is None else ids.to(DEV),
                            n_ids=None if n_ids is None else n_ids.to(DEV), scores=sc, **kw)
    torch.cuda.synchronize()
    return tok.cpu(), (sc.cpu() if scores else None)


def _safe_p(x, keep_k, p):
    """nudge p so that no value group's mass-above lies within 1e-5 of it"""
    above = np.sort(R.mass_above(np.where(keep_k, x, -np.inf))[keep_k])
    for _ in range(200):
        if np.min(np.abs(above - p)) > 1e-5:
            return p
        p = p - 3e-5
    raise AssertionError("no safe p")


@pytest.mark.parametrize("V", [3000, 152064, 152063])
@pytest.mark.parametrize("rows", [1, 8, 33])
@pytest.mark.parametrize("mode", list(MODES))
def test_kernel_matches_oracle(V, rows, mode):
    _need_gpu()
    pen, T, k, ex, p = MODES[mode]
    if k >= V:
        k = V // 3
    lg = _rows(rows, V, V + rows, peak=16.0 if p < 1.0 else 0.0)
    ids = _ids(rows, V, rows)
    n_ids = torch.randint(0, ids.shape[1] + 1, (rows,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    u = torch.rand(rows, generator=torch.Generator().manual_seed(11))
    ps = []
    for r in range(rows):
        x = R.process(lg[r].numpy(), penalty=pen, ids=ids[r, :n_ids[r]].numpy(), temperature=T)[0]
        _, keep_k = R.process(lg[r].numpy(), penalty=pen, ids=ids[r, :n_ids[r]].numpy(), temperature=T, top_k=k, exact_k=ex)
        ps.append(_safe_p(x, keep_k, p) if p < 1.0 else 1.0)
    # one launch per distinct p (rows share one p per launch): group rows by their safe p
    for pv in sorted(set(ps)):
        sel = [r for r in range(rows) if ps[r] == pv]
        tok, sc = _run(lg[sel], u=u[sel], ids=ids[sel], n_ids=n_ids[sel], temperature=T, top_k=k, exact_k=ex, top_p=pv, penalty=pen)
        for j, r in enumerate(sel):
            want, keep = R.process(lg[r].numpy(), penalty=pen, ids=ids[r, :n_ids[r]].numpy(), temperature=T, top_k=k, exact_k=ex, top_p=pv)
            got = sc[j].numpy()
            assert np.array_equal(np.isfinite(got), keep), (mode, r, int(np.isfinite(got).sum()), int(keep.sum()))
            np.testing.assert_array_equal(got[keep], want[keep])
            t, dist = R.draw(want, float(u[r]))
            if dist > 1e-6:
                assert int(tok[j]) == t, (mode, r, int(tok[j]), t)
            assert keep[int(tok[j])]


def test_distribution_on_a_u_grid():
    _need_gpu()
    V, n = 3000, 4096
    base = _rows(1, V, 77)[0]
    base[:40] += 6.0                                        # a few dozen ids carry most of the mass
    lg = base[None].expand(n, V).contiguous()
    u = (torch.arange(n, dtype=torch.float64) + 0.5) / n
    for kw in ({"temperature": 0.8, "top_k": 20, "top_p": 0.8}, {"top_p": 0.95}, {"top_k": 30, "exact_k": True}):
        tok, _ = _run(lg, u=u.float(), scores=False, **kw)
        want, _ = R.process(base.numpy(), **kw)
        prob = R.probs(want)
        freq = np.bincount(tok.numpy(), minlength=V) / n
        assert np.max(np.abs(freq - prob)) <= 1.0 / n + 1e-6, kw


def test_edges():
    _need_gpu()
    V = 152064
    lg = _rows(4, V, 5)
    tok, sc = _run(lg, u=torch.rand(4), top_k=1)
    assert tok.tolist() == lg.argmax(-1).tolist() and int(torch.isfinite(sc).sum()) == 4
    tok, sc = _run(lg, u=torch.rand(4), top_p=1e-7)
    assert tok.tolist() == lg.argmax(-1).tolist() and int(torch.isfinite(sc).sum()) == 4
    one = torch.full((2, V), float("-inf"))
    one[0, 12345] = 3.0
    one[1, V - 1] = -2.0
    for kw in ({}, {"top_k": 50}, {"top_p": 0.5}, {"top_k": 50, "exact_k": True, "temperature": 0.5}):
        tok, _ = _run(one, u=torch.tensor([0.999, 0.0]), **kw)
        assert tok.tolist() == [12345, V - 1], kw
    # ties at the k-th value: HF keeps all of them, exact mode cuts by id
    t = torch.randn(1, V) - 10.0
    t[0, [5, 900, 70000, 150000]] = 4.0
    t[0, 3] = 6.0
    _, sc = _run(t, u=torch.tensor([0.5]), top_k=2)
    assert torch.isfinite(sc[0]).nonzero().view(-1).tolist() == [3, 5, 900, 70000, 150000]
    _, sc = _run(t, u=torch.tensor([0.5]), top_k=3, exact_k=True)
    assert torch.isfinite(sc[0]).nonzero().view(-1).tolist() == [3, 5, 900]
    # argmax mode (u = NULL): first index of the maximum, after the penalty
    t[0, 3] = 4.0
    tok, _ = _run(t, scores=False)
    assert tok.tolist() == [3]
    ids = torch.tensor([[3, 3, 5]], dtype=torch.int32)
    tok, _ = _run(t, ids=ids, n_ids=torch.tensor([3], dtype=torch.int32), penalty=1.5, scores=False)
    assert tok.tolist() == [900]


@pytest.mark.parametrize("cfgw", [3.0, 1.3])
def test_exact_mode_with_cfg_agrees_with_sample_topk(cfgw):
    _need_gpu()
    from audio_intelligence_amd import _lib as L
    lib = L.lib()
    V, rows, k, T = 8200, 8, 48, 0.8
    g = torch.Generator().manual_seed(9)
    lg, cl = torch.randn(rows, V, generator=g) * 2, torch.randn(rows, V, generator=g) * 2
    iv = torch.tensor([[[s * 1025, (s + 1) * 1025], [0, 0]] for s in range(rows)], dtype=torch.int32)
    u = torch.rand(rows, generator=g)
    d = lambda t: t.to(DEV).contiguous()
    lgd, cld, ivd = d(lg), d(cl), d(iv)
    o_idx = torch.empty((rows, k), dtype=torch.int32, device=DEV)
    o_prob = torch.empty((rows, k), dtype=torch.float32, device=DEV)
    a = L.SampleArgs()
    a.logits, a.cfg_logits, a.cfg, a.rows, a.ld, a.one_minus_cfg = lgd.data_ptr(), cld.data_ptr(), cfgw, rows, V, float(1.0 - cfgw)
    a.allowed, a.n_iv, a.k, a.temperature, a.model_dtype = ivd.data_ptr(), 2, k, T, L.F32
    a.topk_idx, a.topk_prob = o_idx.data_ptr(), o_prob.data_ptr()
    L.check(lib.afhip_sample_topk(C.byref(a), L.stream_ptr()))
    from audio_intelligence_amd import ops
    sc = torch.empty((rows, V), device=DEV)
    tok = ops.sample_filter(lgd, temperature=T, top_k=k, exact_k=True, allowed=ivd, cfg_logits=cld, cfg=cfgw, u=d(u), scores=sc)
    torch.cuda.synchronize()
    for r in range(rows):
        kept = torch.isfinite(sc[r]).nonzero().view(-1).cpu()
        assert sorted(o_idx[r].cpu().tolist()) == kept.tolist()
        p = torch.softmax(sc[r].double(), 0)[o_idx[r].long()].cpu().float()
        np.testing.assert_allclose(p.numpy(), o_prob[r].cpu().numpy(), atol=1e-6, rtol=1e-5)
        assert int(tok[r]) in kept.tolist()


def test_bitwise_determinism_and_graph_replay():
    _need_gpu()
    from audio_intelligence_amd import ops
    V, rows = 152064, 16
    lg = _rows(rows, V, 123).to(DEV)
    u = torch.rand(rows, generator=torch.Generator().manual_seed(1)).to(DEV)
    ids = _ids(rows, V, 4).to(DEV)
    n_ids = torch.full((rows,), ids.shape[1], dtype=torch.int32, device=DEV)
    kw = dict(temperature=0.7, top_k=20, top_p=0.8, penalty=1.05, penalty_ids=ids, n_ids=n_ids, u=u)
    outs = []
    for _ in range(2):
        sc = torch.empty((rows, V), device=DEV)
        outs.append((ops.sample_filter(lg, scores=sc, **kw), sc))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    kw2 = dict(temperature=1.0, top_p=0.95, u=u)
    sc_e = torch.empty((rows, V), device=DEV)
    tok_e = ops.sample_filter(lg, scores=sc_e, **kw2)
    sc_g = torch.empty((rows, V), device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.sample_filter(lg, scores=sc_g, **kw2)                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tok_g = ops.sample_filter(lg, scores=sc_g, **kw2)
    sc_g.fill_(0.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(tok_g, tok_e) and torch.equal(sc_g.view(torch.int32), sc_e.view(torch.int32))
