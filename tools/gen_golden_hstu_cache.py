#!/usr/bin/env python3
"""Golden vectors for the HSTU encoder's cached incremental decoding: runs the REFERENCE's own prefill
(`encode(..., return_cache_states=True)`) and decode (`encode(..., delta_x_offsets=..., cache=...)`, modeling/sequential/hstu.py) on the
CPU and writes tests/golden/hstu_cache_<config>.npz.

TEST INFRASTRUCTURE ONLY.  It imports oracle/gen_golden_hstu.py, which installs the stand-ins for fbgemm's three jagged layout ops
and provides build_reference / make_inputs; the model and the prefill inputs are exactly those of tests/golden/hstu_<config>.npz (same
seeds), so the weights are read from there and not stored again.  Six sequences per geometry (lengths N and 1 among them) and five
scenarios, each decoding one row per sequence:
  tail       prefill, then a new item at lengths - 1 (timestamps unchanged)
  tail2      a second decode at the same positions on the cache `tail` left behind
  interior   prefill, then a new item at a position < lengths - 1 where there is one (the result stays the prefill's)
  ts         like interior, with ts[p] changed for the decode call (the cached rows keep the old bias)
  nots       prefill and decode without timestamps
Stored per scenario: the positions, the decode's ids / timestamps, the prefill's and the decode's current embeddings, and the cache
rows the decode wrote (v / outputs at the jagged rows, q / k at (b, p), every layer).  For ML-1M (the small geometry) the whole cache
after `interior` too; elsewhere the prefill's states at eight sampled jagged rows.
  python tools/gen_golden_hstu_cache.py
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))

import gen_golden_hstu as G  # noqa: E402  (installs the fbgemm layout stand-ins; imports the reference)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from _npz import savez_deterministic  # noqa: E402

from oracle import hstu_oracle as HO  # noqa: E402
from tests import _hstu_cache_ref as R  # noqa: E402

B = 6


def scenario_inputs(cfg, lengths, ids, ts, g, interior: bool):
    N = cfg.max_sequence_len
    if interior:
        pos = torch.stack([torch.randint(0, max(int(l) - 1, 1), (1,), generator=g)[0] for l in lengths])
    else:
        pos = lengths - 1
    new_ids = ids.clone()
    new_ids[torch.arange(B), pos] = torch.randint(1, cfg.num_items + 1, (B,), generator=g)
    return pos.to(torch.int64), new_ids, ts


def run(model, lengths, ids, ts):
    with torch.inference_mode():
        emb = model.get_item_embeddings(ids)
        pay = {"timestamps": ts} if ts is not None else {}
        return model.encode(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads=pay, return_cache_states=True)


def step(model, lengths, ids, ts, pos, cache):
    off = torch.cumsum(lengths, 0) - lengths
    with torch.inference_mode():
        emb = model.get_item_embeddings(ids)
        pay = {"timestamps": ts} if ts is not None else {}
        cur, states = model.encode(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads=pay,
                                   delta_x_offsets=(off + pos, pos), cache=cache, return_cache_states=True)
    assert all(s[0] is c[0] and s[3] is c[3] for s, c in zip(states, cache))    # the cache is updated in place
    return cur, states


def main():
    for name, cfg in HO.HSTU_CONFIGS.items():
        model = G.build_reference(cfg, seed=11)
        lengths, ids, ts = G.make_inputs(cfg, B, seed=5)
        base = np.load(os.path.join(REPO, "tests", "golden", f"hstu_{name}.npz"))
        sd = model.state_dict()
        for k in base.files:
            if k.startswith("w/"):
                assert np.array_equal(base[k], sd[k[2:]].numpy()), k   # same model as the encoder fixture
        w = {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("w/")}
        g = torch.Generator().manual_seed(17)
        arrays = {"in/past_lengths": lengths.numpy(), "in/past_ids": ids.numpy(), "in/timestamps": ts.numpy(),
                  "meta/torch_version": np.array(torch.__version__)}

        def record(tag, pos, new_ids, new_ts, pre_cur, cur, states):
            arrays[f"{tag}/positions"] = pos.numpy()
            arrays[f"{tag}/ids"] = new_ids.numpy()
            if new_ts is not None:
                arrays[f"{tag}/timestamps"] = new_ts.numpy()
            arrays[f"{tag}/prefill_current"] = pre_cur.numpy()
            arrays[f"{tag}/current"] = cur.numpy()
            for k, v in R.touched(states, lengths, pos).items():
                arrays[f"{tag}/{k}"] = v.numpy()

        def check(pre_cur, cur, cur_states, new_ids, new_ts, pos, stamps_prefill, cache_in=None):
            # the restatement (float32, as the reference runs) reproduces the reference before it is trusted
            c, st = R.prefill(cfg, w, lengths, ids, stamps_prefill) if cache_in is None else (None, cache_in)
            if c is not None:
                assert float((c - pre_cur).abs().max()) < 2e-5
            d = R.decode(cfg, w, lengths, new_ids, new_ts, pos, st)
            err = float((d - cur).abs().max())
            rows = max(float((a - b).abs().max()) for a, b in zip(R.touched(st, lengths, pos).values(), R.touched(cur_states, lengths, pos).values()))
            assert err < 2e-5 and rows < 2e-4, (err, rows)
            return st

        # tail, then tail2 on the mutated cache
        pre_cur, cache = run(model, lengths, ids, ts)
        pos, new_ids, _ = scenario_inputs(cfg, lengths, ids, ts, g, interior=False)
        cur, cache = step(model, lengths, new_ids, ts, pos, cache)
        mine = check(pre_cur, cur, cache, new_ids, ts, pos, ts)
        record("tail", pos, new_ids, None, pre_cur, cur, cache)
        ids2 = new_ids.clone()
        ids2[torch.arange(B), pos] = torch.randint(1, cfg.num_items + 1, (B,), generator=g)
        cur2, cache = step(model, lengths, ids2, ts, pos, cache)
        check(cur, cur2, cache, ids2, ts, pos, ts, cache_in=mine)
        record("tail2", pos, ids2, None, cur, cur2, cache)
        # interior; a changed ts[p]; no timestamps
        for tag in ("interior", "ts", "nots"):
            stamps = None if tag == "nots" else ts
            pre_cur, cache = run(model, lengths, ids, stamps)
            if tag == "interior" and name != "ml-1m":
                sample = torch.randperm(int(lengths.sum()), generator=torch.Generator().manual_seed(3))[:8]
                arrays["sample/rows"] = sample.numpy()
                for l, (v, q, k, o) in enumerate(cache):   # copies: the decode below updates the cache in place
                    arrays[f"sample/l{l}/v"], arrays[f"sample/l{l}/outputs"] = v[sample].numpy().copy(), o[sample].numpy().copy()
                    arrays[f"sample/l{l}/q"], arrays[f"sample/l{l}/k"] = q[0].numpy().copy(), k[0].numpy().copy()   # the full-length sequence
            pos, new_ids, _ = scenario_inputs(cfg, lengths, ids, ts, g, interior=tag != "nots")
            new_ts = stamps
            if tag == "ts":
                new_ts = ts.clone()
                new_ts[torch.arange(B), pos] += torch.randint(1, 10 ** 6, (B,), generator=g)
            cur, cache = step(model, lengths, new_ids, new_ts, pos, cache)
            check(pre_cur, cur, cache, new_ids, new_ts, pos, stamps)
            record(tag, pos, new_ids, new_ts if tag == "ts" else None, pre_cur, cur, cache)
            if tag == "interior" and name == "ml-1m":
                for l, (v, q, k, o) in enumerate(cache):
                    arrays[f"full/l{l}/v"], arrays[f"full/l{l}/q"], arrays[f"full/l{l}/k"], arrays[f"full/l{l}/outputs"] = (
                        v.numpy().copy(), q.numpy().copy(), k.numpy().copy(), o.numpy().copy())
        path = os.path.join(REPO, "tests", "golden", f"hstu_cache_{name}.npz")
        savez_deterministic(path, **arrays)
        print(f"{name}: wrote tests/golden/hstu_cache_{name}.npz ({os.path.getsize(path) // 1024} KB)")


if __name__ == "__main__":
    main()
