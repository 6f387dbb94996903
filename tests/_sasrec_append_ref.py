"""float64 restatement of SASRec's multi-row cached decode step (SASRec.encode with cache= and new_rows=) for the append tests.

`append64` is the definition: the single-row float64 step (tests/_sasrec_decode_ref.step64) applied to rows len - m .. len - 1 of
every sequence in order.  `rows64` restates the step the way the kernels run it -- B * M work-row slots, all of a block's new k / v
rows written before that block's attention, each row attending to keys 0 .. p_r -- so that the tests can check that the two forms
agree, and that the bars reject the mistakes a multi-row implementation can make (`bug`, one of BUGS)."""
import torch

from tests import _sasrec_decode_ref as R
from tests import _sasrec_ref as S

BUGS = [
    "blind_to_earlier_new_rows",   # a new row attends to the cache as it was before the step, plus its own k / v
    "sees_later_new_rows",         # every new row's key limit is the sequence's last row
    "last_pos_for_all",            # the position embedding of row len - 1 for every new row
    "shift_down",                  # the first new row one too low: rows len - m - 1 .. len - 2
    "shift_up",                    # ... one too high: rows len - m + 1 .. len
    "skips_first_new_row",         # the first new row one too high with the last one in place: row len - m is never re-encoded
    "inactive_slot_writes",        # a slot t >= m_b writes the k / v of its zero row to cache row min(len - m + t, N - 1)
]


def fixture_step(f, first=0, last=3):
    """The one step from the fixture chain's state `first` to state `last`: (lengths, ids, counts) with counts[b] = the length at
    `last` minus the first row at which the two states' ids differ."""
    L, I = torch.from_numpy(f["chain/lengths"]), torch.from_numpy(f["chain/ids"])
    diff = I[first] != I[last]
    assert bool(diff.any(1).all())
    return L[last], I[last], L[last] - diff.int().argmax(1)


def single_steps(lengths, counts):
    """The lengths of the M single-row steps that one multi-row step equals: step s runs at len - m + 1 + min(s, m - 1) (a sequence
    with fewer than M new rows re-encodes its last row again, which changes nothing)."""
    M = int(counts.max())
    return [lengths - counts + 1 + torch.clamp(torch.full_like(counts, s), max=counts - 1) for s in range(M)]


def append64(f, cache, lengths, ids, counts):
    """(current (B, D), the updated cache): step64 over rows len - m .. len - 1 in order.  `cache` is not modified."""
    for L in single_steps(lengths, counts):
        cur, cache = R.step64(f, cache, L, ids)
    return cur, cache


def rows64(f, cache, lengths, ids, counts, M=None, bug=None):
    """The same step block by block over B * M slots.  `cache` is not modified."""
    c, w = f["cfg"], R.weights(f)
    B, N = ids.shape
    D, H = c["D"], c["heads"]
    hd = D // H
    M = int(counts.max()) if M is None else M
    cache = [(k.clone(), v.clone()) for k, v in cache]
    emb, pos = w["_embedding_module._item_emb.weight"], w["_input_features_preproc._pos_emb.weight"]
    out = torch.empty((B, D), dtype=torch.float64)
    for b in range(B):
        L, m = int(lengths[b]), int(counts[b])
        if bug == "skips_first_new_row" and m > 1:
            m -= 1
        shift = {"shift_down": -1, "shift_up": 1}.get(bug, 0)
        rows = [min(max(L - m + t + shift, 0), N - 1) for t in range(m)]          # the active slots' positions
        ghosts = [min(L - m + t, N - 1) for t in range(m, M)] if bug == "inactive_slot_writes" else []
        keep = [1.0 if int(ids[b, p]) != 0 else 0.0 for p in rows]
        xs = [(emb[int(ids[b, p])] * float(D) ** 0.5 + pos[rows[-1] if bug == "last_pos_for_all" else p]) * k for p, k in zip(rows, keep)]
        for i in range(c["blocks"]):
            a, pf = f"attention_layers.{i}.", f"forward_layers.{i}._conv1d."
            W, bias = w[a + "in_proj_weight"], w[a + "in_proj_bias"]
            kc, vc = cache[i]
            k_old, v_old = kc[b].clone(), vc[b].clone()
            Qs = [S._ln(x, 1e-8) for x in xs]
            kvs = [x @ W[D:].T + bias[D:] for x in xs]
            for p, kv in zip(rows, kvs):                       # every new row's k / v, before any attention
                kc[b, p], vc[b, p] = kv[:D], kv[D:]
            for p in ghosts:                                   # a zero row's k / v: the bias
                kc[b, p], vc[b, p] = bias[D:2 * D], bias[2 * D:]
            for t, p in enumerate(rows):
                top = rows[-1] if bug == "sees_later_new_rows" else p
                if bug == "blind_to_earlier_new_rows":
                    keys, vals = k_old[:p + 1].clone(), v_old[:p + 1].clone()
                    keys[p], vals[p] = kvs[t][:D], kvs[t][D:]
                else:
                    keys, vals = kc[b, :top + 1], vc[b, :top + 1]
                q = Qs[t] @ W[:D].T + bias[:D]
                att = torch.empty(D, dtype=torch.float64)
                for h in range(H):
                    sl = slice(h * hd, (h + 1) * hd)
                    att[sl] = torch.softmax(keys[:, sl] @ q[sl] / hd ** 0.5, 0) @ vals[:, sl]
                z = S._ln(Qs[t] + att @ w[a + "out_proj.weight"].T + w[a + "out_proj.bias"], 1e-8)
                xs[t] = R._ffn(w, pf, z, c["act"]) * keep[t]
        out[b] = R._post(xs[-1], c["postproc"])
    return out, cache
