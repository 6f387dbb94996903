#!/usr/bin/env python3
"""Golden vectors for the HSTU encoder's multi-row cached decode step (HSTU.encode(..., delta_rows=)): runs the REFERENCE's own
prefill and its own single-row decode (`encode(..., delta_x_offsets=..., cache=...)`, modeling/sequential/hstu.py), chained over the
rows of a run in ascending order, on the CPU and writes tests/golden/hstu_rows_<config>.npz.

TEST INFRASTRUCTURE ONLY.  Like tools/gen_golden_hstu_cache.py it imports oracle/gen_golden_hstu.py (the fbgemm layout stand-ins,
build_reference / make_inputs); model and base inputs are those of tests/golden/hstu_<config>.npz.  Six sequences, two scenarios:
  edit     prefill, then the last m_b <= 3 rows of every sequence get new ids and are decoded one row per step, in ascending order (a
           sequence whose run is over repeats its last row: the same inputs, the same bits)
  append   prefill at the old lengths (ids and timestamps zero past them, as a caller's padding is), the cache laid out for the new
           lengths (old rows moved, new rows zero: row movement only, tests/_hstu_rows_ref.py:extend_states), then the run
           [len_old - 1, len_new) decoded one row per step; and the reference's own prefill at the new lengths
Stored: the inputs, the runs, the results, and the cache rows of the runs (v / outputs at the jagged rows, q / k at (b, p), every
layer) after the chain -- for `append` those rows of the prefill at the new lengths as well.
  python tools/gen_golden_hstu_decode_rows.py
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
from tests import _hstu_rows_ref as M  # noqa: E402
from gen_golden_hstu_cache import run, step  # noqa: E402  (tools/ is the script's own directory)

B = 6


def chain(model, lengths, ids, ts, start, counts, cache):
    """The reference's single-row decode at start + t, t = 0 .. max(counts) - 1; a finished sequence repeats its last row."""
    cur = None
    for t in range(int(counts.max())):
        cur, cache = step(model, lengths, ids, ts, start + torch.minimum(torch.full_like(counts, t), counts - 1), cache)
    return cur, cache


def main():
    for name, cfg in HO.HSTU_CONFIGS.items():
        N = cfg.max_sequence_len
        model = G.build_reference(cfg, seed=11)
        lengths, ids, ts = G.make_inputs(cfg, B, seed=5)
        base = np.load(os.path.join(REPO, "tests", "golden", f"hstu_{name}.npz"))
        w = {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("w/")}
        sd = model.state_dict()
        assert all(np.array_equal(base["w/" + k], sd[k].numpy()) for k in w)       # same model as the encoder fixture
        g = torch.Generator().manual_seed(23)
        arrays = {"in/past_lengths": lengths.numpy(), "in/past_ids": ids.numpy(), "in/timestamps": ts.numpy(),
                  "meta/torch_version": np.array(torch.__version__)}

        def check(cur, states, lens, new_ids, start, counts, mine):
            # the restatement (float32, as the reference runs) reproduces the reference before it is trusted
            c = M.chain(cfg, w, lens, new_ids, ts, start, counts, mine)
            rows = max(float((a - b).abs().max()) for a, b in zip(M.touched(mine, lens, start, counts).values(),
                                                                  M.touched(states, lens, start, counts).values()))
            assert float((c - cur).abs().max()) < 2e-5 and rows < 2e-4, (float((c - cur).abs().max()), rows)

        # ---- edit: the last m_b rows, m_b in {1, 2, 3}
        counts = torch.minimum(1 + (torch.arange(B) + 2) % 3, lengths)
        start = lengths - counts
        new_ids = ids.clone()
        b, p = M.run_rows(lengths, start, counts)
        new_ids[b, p] = torch.randint(1, cfg.num_items + 1, (b.numel(),), generator=g)
        pre_cur, cache = run(model, lengths, ids, ts)
        mine = R.prefill(cfg, w, lengths, ids, ts)[1]
        cur, cache = chain(model, lengths, new_ids, ts, start, counts, cache)
        check(cur, cache, lengths, new_ids, start, counts, mine)
        arrays.update({"edit/start": start.numpy(), "edit/counts": counts.numpy(), "edit/ids": new_ids.numpy(),
                       "edit/prefill_current": pre_cur.numpy(), "edit/current": cur.numpy()})
        for k, v in M.touched(cache, lengths, start, counts).items():
            arrays[f"edit/{k}"] = v.numpy().copy()

        # ---- append: one or two events per sequence
        grow = 1 + torch.arange(B) % 2
        old = torch.where(lengths + grow > N, N - grow, lengths)
        new = old + grow
        valid_new = torch.arange(N).unsqueeze(0) < new.unsqueeze(1)
        valid_old = torch.arange(N).unsqueeze(0) < old.unsqueeze(1)
        ids_new = torch.where(valid_new & (ids == 0), torch.randint(1, cfg.num_items + 1, (B, N), generator=g), ids) * valid_new
        ids_old, ts_old = ids_new * valid_old, ts * valid_old
        _, cache = run(model, old, ids_old, ts_old)
        mine = M.extend_states(R.prefill(cfg, w, old, ids_old, ts_old)[1], old, new)
        cache = M.extend_states(cache, old, new)
        start, counts = old - 1, grow + 1
        cur, cache = chain(model, new, ids_new, ts, start, counts, cache)
        check(cur, cache, new, ids_new, start, counts, mine)
        full_cur, full = run(model, new, ids_new, ts)
        arrays.update({"append/old_lengths": old.numpy(), "append/new_lengths": new.numpy(), "append/ids": ids_new.numpy(),
                       "append/current": cur.numpy(), "append/prefill_current": full_cur.numpy()})
        for k, v in M.touched(cache, new, start, counts).items():
            arrays[f"append/{k}"] = v.numpy().copy()
        for k, v in M.touched(full, new, start, counts).items():
            arrays[f"append/prefill_{k}"] = v.numpy().copy()
        path = os.path.join(REPO, "tests", "golden", f"hstu_rows_{name}.npz")
        savez_deterministic(path, **arrays)
        print(f"{name}: wrote tests/golden/hstu_rows_{name}.npz ({os.path.getsize(path) // 1024} KB); "
              f"append chain vs prefill at the new lengths: {float((cur - full_cur).abs().max()):.2e}")


if __name__ == "__main__":
    main()
