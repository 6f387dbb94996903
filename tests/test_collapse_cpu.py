"""CPU: the host side of collapse_groups=True -- the three entry points in header, binding and library under ABI 15, the
group-key row under edits against a brute-force model, the dense ranks the kernels read, and the sanity of the reference walk the GPU tests
compare with (tests/_collapse_ref.py)."""
import os
import re

import torch

from rails_amd import _lib
from rails_amd import topk_modules as T
from tests import _collapse_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rails_topk_collapse", "rails_scores_group_max", "rails_topk_keys")


def header_text():
    with open(os.path.join(ROOT, "include", "rails_amd.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_entry_points_are_declared_bound_and_exported_under_abi_15():
    header = header_text()
    lib = _lib.load()
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m is not None, f"{name} is not declared in include/rails_amd.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.PROTOTYPES, f"{name} is not bound in rails_amd/_lib.py"
        assert len(_lib.PROTOTYPES[name][1]) == n_args, (name, n_args, len(_lib.PROTOTYPES[name][1]))
        assert getattr(lib, name) is not None
    assert re.search(r"#define\s+RAILS_ABI_VERSION\s+15\b", header)
    assert _lib.RAILS_ABI_VERSION == 15 and lib.rails_abi_version() == 15


def model_after_removal(row, positions):
    """remove_items by its definition, one list operation at a time: the removed positions below N' are holes, filled in ascending order by the
    surviving positions at or above N' in ascending order."""
    n, gone = len(row), set(positions)
    n_new = n - len(gone)
    holes = sorted(p for p in gone if p < n_new)
    movers = [p for p in range(n_new, n) if p not in gone]
    out = list(row[:n_new])
    for h, m in zip(holes, movers):
        out[h] = row[m]
    return out


def test_group_rows_follow_edits_as_a_brute_force_model_does():
    g = torch.Generator().manual_seed(71)
    for trial in range(40):
        n = int(torch.randint(2, 200, (1,), generator=g))
        row = torch.randint(-1, 12, (n,), generator=g).to(torch.int32)
        m = int(torch.randint(0, n, (1,), generator=g))      # (at least one item stays)
        pos = torch.randperm(n, generator=g)[:m]
        holes, movers = T.removal_plan(pos, n)
        got = T.groups_after_removal(row, n - m, holes, movers)
        assert got.dtype == torch.int32 and got.tolist() == model_after_removal(row.tolist(), pos.tolist()), trial
        assert got.data_ptr() != row.data_ptr()
        extra = int(torch.randint(1, 40, (1,), generator=g))
        grown = T.groups_after_append(got, n - m, n - m + extra)
        assert grown.dtype == torch.int32 and grown.tolist() == got.tolist() + [-1] * extra, trial


def same_partition(ranks, keys):
    """ranks collapse exactly what the keys collapse: equal keys >= 0 <-> equal ranks, and a -1 item shares its rank with nobody."""
    by_rank = {}
    for p, r in enumerate(ranks):
        by_rank.setdefault(r, []).append(p)
    for members in by_rank.values():
        ks = {keys[p] for p in members}
        if len(members) > 1:
            assert len(ks) == 1 and -1 not in ks, (members, ks)
    by_key = {}
    for p, key in enumerate(keys):
        if key >= 0:
            by_key.setdefault(key, set()).add(ranks[p])
    assert all(len(r) == 1 for r in by_key.values())


def test_dense_ranks():
    g = torch.Generator().manual_seed(72)
    for dtype in (torch.int32, torch.int64):
        keys = torch.tensor([5, -1, 5, (1 << 31) - 2, -1, 0, (1 << 31) - 2, 7], dtype=dtype)
        ranks, groups = T.group_ranks(keys)
        assert ranks.dtype == torch.int32 and ranks.shape == keys.shape
        assert groups == 6 and sorted(set(ranks.tolist())) == list(range(6))
        same_partition(ranks.tolist(), keys.tolist())
    only = T.group_ranks(torch.full((9,), 3, dtype=torch.int32))
    assert only[1] == 1 and only[0].tolist() == [0] * 9
    none = T.group_ranks(torch.full((9,), -1, dtype=torch.int32))
    assert none[1] == 9 and sorted(none[0].tolist()) == list(range(9))
    # an edit chain: the ranks of the row the chain leaves collapse what its keys collapse, G <= N, and are those of the same row built afresh
    row = torch.randint(-1, 30, (150,), generator=g).to(torch.int32)
    for step in range(6):
        n = row.numel()
        if step % 2 == 0:
            pos = torch.randperm(n, generator=g)[: n // 5]
            holes, movers = T.removal_plan(pos, n)
            row = T.groups_after_removal(row, n - pos.numel(), holes, movers)
        else:
            row = T.groups_after_append(row, n, n + 17)
            row[n : n + 5] = torch.tensor([2, 2, 29, 31, 31], dtype=torch.int32)      # (set_item_groups(..., positions) on some of the new items)
        ranks, groups = T.group_ranks(row)
        assert groups <= row.numel() and int(ranks.min()) == 0 and int(ranks.max()) == groups - 1
        same_partition(ranks.tolist(), row.tolist())
        fresh = T.group_ranks(row.clone())
        assert fresh[1] == groups and torch.equal(fresh[0], ranks)


def test_reference_walk_properties():
    g = torch.Generator().manual_seed(73)
    for trial in range(30):
        n = int(torch.randint(5, 300, (1,), generator=g))
        scores = torch.randint(-4, 5, (n,), generator=g).float()      # small integers: ties abound, the position rule decides
        scores[torch.rand(n, generator=g) < 0.1] = float("-inf")
        keys = torch.randint(-1, max(2, n // 4), (n,), generator=g)
        ids = torch.randperm(n, generator=g) * 3 + 1
        invalid = ids[torch.randperm(n, generator=g)[: n // 6]]
        k = int(torch.randint(1, n, (1,), generator=g))
        order = CR.key_order(scores)
        assert sorted(order.tolist()) == list(range(n))
        ranked = [(scores[p].item(), p) for p in order.tolist()]
        assert all(a[0] > b[0] or (a[0] == b[0] and a[1] < b[1]) for a, b in zip(ranked, ranked[1:]))
        s, pos, out_ids = CR.collapse_walk(scores, order, keys, invalid, ids, k)
        assert len(pos) <= k and [ids[p].item() for p in pos] == out_ids and [scores[p].item() for p in pos] == s
        where = {p: j for j, p in enumerate(order.tolist())}
        assert all(where[a] < where[b] for a, b in zip(pos, pos[1:]))                       # a subsequence of the order
        kept_keys = [keys[p].item() for p in pos if keys[p] >= 0]
        assert len(kept_keys) == len(set(kept_keys))                                        # no two outputs share a non-negative key
        bad = set(invalid.tolist())
        assert all(scores[p] > float("-inf") and ids[p].item() not in bad for p in pos)     # only eligible items
        last = where[pos[-1]] if len(pos) == k else n                                       # the walk stopped behind its k-th output
        kept = set(pos)
        for p in order.tolist()[: last]:
            eligible = scores[p] > float("-inf") and ids[p].item() not in bad
            if eligible and p not in kept:                                                  # every skipped eligible item has an earlier kept item of its group
                assert keys[p] >= 0 and any(keys[o] == keys[p] and where[o] < where[p] for o in pos), (trial, p)


def test_ungrouped_corpus_walk_is_the_plain_ranking():
    scores = torch.tensor([1.0, 3.0, 3.0, -2.0, 0.0, float("-inf")])
    s, pos, ids = CR.collapse_walk(scores, CR.key_order(scores), torch.full((6,), -1), None, None, 4)
    assert pos == [1, 2, 0, 4] and ids == pos and s == [3.0, 3.0, 1.0, 0.0]
    one = CR.collapse_walk(scores, CR.key_order(scores), torch.zeros(6, dtype=torch.int64), None, None, 2)
    assert one[1] == [1]                                                                    # one group: one result, however many are asked for
