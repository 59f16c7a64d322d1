"""Host restatement of transformers' beam search (GenerationMixin._beam_search: steps b-g, the early-stop heuristic, the loop condition,
finalisation and cropping), driven by a callback that returns each step's logits for the running sequences.  Pinned to transformers'
own generate(num_beams=...) by tests/test_beam_ref_host.py; replays the GPU's generate() in tests/test_gpu_beam_search.py."""
from types import SimpleNamespace

import torch


def _take(t, idx):
    return torch.take_along_dim(t, idx.view(idx.shape + (1,) * (t.dim() - 2)), dim=1)


def beam_search(logits_fn, input_ids, vocab_size, num_beams, max_new_tokens, eos=(), pad=None, length_penalty=1.0, early_stopping=False,
                num_return_sequences=1):
    """logits_fn(step, running [B * nb, cur_len] int64) -> [B * nb, V] logits of the next token of every running sequence.
    Returns sequences [B * nrs, W + n], sequences_scores [B * nrs], beam_indices [B * nrs, n], the per-step log-prob rows `scores`,
    and `margin`: the smallest gap, over every step and prompt, between neighbours among the K + 1 best accumulated candidates and
    among the values steps e / f rank (a replay whose logits differ by less than that cannot choose differently)."""
    eos = list(eos)
    B, W = input_ids.shape
    nb, V = num_beams, vocab_size
    max_length = W + max_new_tokens
    K = max(2, 1 + len(eos)) * nb
    top_nb = torch.arange(K) < nb
    fill = ((pad if pad else eos[0]) if eos else -1)
    run_seq = torch.full((B, nb, max_length), fill, dtype=torch.int64)
    run_seq[:, :, :W] = input_ids[:, None]
    seqs = run_seq.clone()
    run_sc = torch.zeros((B, nb))
    run_sc[:, 1:] = -1e9
    fin_sc = torch.full((B, nb), -1e9)
    done = torch.zeros((B, nb), dtype=torch.bool)
    improvable = torch.ones((B, 1), dtype=torch.bool)
    run_bi = torch.full((B, nb, max_length - W), -1, dtype=torch.int32)
    fin_bi = run_bi.clone()
    scores, margin = [], float("inf")
    cur = W

    def gaps(x, n):                     # smallest gap between neighbours among the n largest (values <= -1e8 are dead beams: left out)
        x = x.double()
        s = torch.sort(torch.where(x > -1e8, x, torch.full_like(x, -float("inf"))), dim=-1, descending=True)[0][:, :n]
        d = (s[:, :-1] - s[:, 1:]).flatten()
        d = d[torch.isfinite(d)]
        return float(d.min()) if d.numel() else float("inf")

    while True:
        logits = logits_fn(cur - W, run_seq[:, :, :cur].reshape(B * nb, cur)).to(torch.float32)
        logp = torch.log_softmax(logits, dim=-1)
        scores.append(logp)
        acc = (logp.view(B, nb, V) + run_sc[:, :, None]).reshape(B, nb * V)
        margin = min(margin, gaps(acc, K + 1))
        top_v, top_i = torch.topk(acc, k=K)
        src = top_i // V
        t_seq = _take(run_seq, src)
        t_seq[:, :, cur] = top_i % V
        t_bi = _take(run_bi, src)
        t_bi[:, :, cur - W] = (src + torch.arange(B)[:, None] * nb).to(torch.int32)
        hit = torch.isin(t_seq[:, :, cur], torch.tensor(eos, dtype=torch.int64)) if eos else torch.zeros((B, K), dtype=torch.bool)
        if cur + 1 >= max_length:
            hit = torch.ones_like(hit)
        live = top_v + hit.to(torch.float32) * -1.0e9
        margin = min(margin, gaps(live, nb + 1))
        nxt = torch.topk(live, k=nb)[1]
        run_seq, run_sc, run_bi = _take(t_seq, nxt), _take(live, nxt), _take(t_bi, nxt)
        just = hit & top_nb[None, :]
        cand = top_v / ((cur + 1 - W) ** length_penalty)
        cand = cand + (done.all(-1, keepdim=True) & (early_stopping is True)).to(torch.float32) * -1.0e9
        cand = cand + (~improvable).to(torch.float32) * -1.0e9
        cand = cand + (~just) * -1.0e9
        merged = torch.cat((fin_sc, cand), 1)
        margin = min(margin, gaps(merged, nb + 1))
        keep = torch.topk(merged, k=nb)[1]
        seqs = _take(torch.cat((seqs, t_seq), 1), keep)
        fin_sc = _take(merged, keep)
        fin_bi = _take(torch.cat((fin_bi, t_bi), 1), keep)
        done = _take(torch.cat((done, just), 1), keep)
        cur += 1
        best_len = (max_length if early_stopping == "never" and length_penalty > 0.0 else cur) - W
        worst = torch.where(done, fin_sc.min(1, keepdim=True)[0], -1.0e9)
        improvable = improvable & (run_sc[:, :1] / (best_len ** length_penalty) > worst).any(-1, keepdim=True)
        if not bool(improvable.any() & ~(done.all() & (early_stopping is True)) & ~hit.all()):
            break
    nrs = num_return_sequences
    seqs = seqs[:, :nrs].reshape(B * nrs, -1)
    fin_sc = fin_sc[:, :nrs].reshape(B * nrs)
    fin_bi = fin_bi[:, :nrs].reshape(B * nrs, -1)
    n = int((fin_bi + 1).bool().sum(1).max())
    return SimpleNamespace(sequences=seqs[:, :W + n], sequences_scores=fin_sc, beam_indices=fin_bi[:, :n], scores=scores, margin=margin)
