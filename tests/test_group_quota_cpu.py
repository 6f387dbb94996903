"""CPU: the host side of max_per_group=m -- the reference walk the GPU tests compare with (tests/_quota_ref.py) against
its own properties and against _collapse_ref at m = 1, the numpy model of the fallback's round table against that walk, the two new entry
points in header, binding and library under ABI 15, and every argument check and refusal, message by message, none of which launches."""
import os
import re
import types

import numpy as np
import pytest
import torch

from rails_amd import _lib
from rails_amd import engine as E
from rails_amd import topk_modules as T
from tests import _collapse_ref as CR
from tests import _quota_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("rails_topk_collapse_quota", "rails_scores_group_next")
NEG_INF = float("-inf")


def random_row(g, n, all_tie=False):
    scores = torch.zeros(n) if all_tie else torch.randint(-4, 5, (n,), generator=g).float()      # small integers: ties abound
    scores[torch.rand(n, generator=g) < 0.1] = NEG_INF
    keys = torch.randint(-1, max(2, n // 4), (n,), generator=g)
    ids = torch.randperm(n, generator=g) * 3 + 1
    invalid = ids[torch.randperm(n, generator=g)[: n // 6]]
    return scores, keys, ids, invalid


def test_m_1_is_the_collapse_reference():
    g = torch.Generator().manual_seed(101)
    for trial in range(40):
        n = int(torch.randint(5, 300, (1,), generator=g))
        scores, keys, ids, invalid = random_row(g, n, all_tie=trial % 4 == 3)
        k = int(torch.randint(1, n + 1, (1,), generator=g))
        order = CR.key_order(scores)
        for inv in (None, invalid):
            assert QR.quota_walk(scores, order, keys, inv, ids, k, 1) == CR.collapse_walk(scores, order, keys, inv, ids, k), trial


def test_reference_properties():
    g = torch.Generator().manual_seed(102)
    for trial in range(40):
        n = int(torch.randint(5, 300, (1,), generator=g))
        scores, keys, ids, invalid = random_row(g, n, all_tie=trial % 5 == 4)
        k = int(torch.randint(1, n + 1, (1,), generator=g))
        m = int(torch.randint(1, 6, (1,), generator=g))
        order = CR.key_order(scores)
        bad = set(invalid.tolist())
        eligible = [p for p in order.tolist() if scores[p] > NEG_INF and ids[p].item() not in bad]
        s, pos, out_ids = QR.quota_walk(scores, order, keys, invalid, ids, k, m)
        assert len(pos) <= k and [ids[p].item() for p in pos] == out_ids and [scores[p].item() for p in pos] == s
        where = {p: j for j, p in enumerate(order.tolist())}
        assert all(where[a] < where[b] for a, b in zip(pos, pos[1:]))                       # the output's order is the ranking's
        assert set(pos) <= set(eligible)                                                    # only eligible items
        per_group = {}
        for p in pos:
            if keys[p] >= 0:
                per_group[keys[p].item()] = per_group.get(keys[p].item(), 0) + 1
        assert all(c <= m for c in per_group.values())                                      # never more than m of a group
        # by the definition, item by item: a survivor has fewer than m eligible predecessors of its key, the first k of them are the output
        survivors = [p for j, p in enumerate(eligible) if keys[p] < 0 or sum(1 for o in eligible[:j] if keys[o] == keys[p]) < m]
        assert pos == survivors[:k], trial
        # every group no larger than m: the plain eligible ranking
        big = max(int(torch.bincount(keys[keys >= 0]).max()) if bool((keys >= 0).any()) else 1, 1)
        assert QR.quota_walk(scores, order, keys, invalid, ids, k, big)[1] == eligible[:k]
        assert QR.quota_walk(scores, order, torch.full((n,), -1), invalid, ids, k, m)[1] == eligible[:k]


def test_a_seen_member_frees_its_slot():
    scores = torch.tensor([9.0, 8.0, 7.0, 6.0, 5.0, 4.0])
    keys = torch.tensor([0, 0, 0, 0, 1, -1])
    ids = torch.tensor([10, 11, 12, 13, 14, 15])
    order = CR.key_order(scores)
    assert QR.quota_walk(scores, order, keys, None, ids, 6, 2)[2] == [10, 11, 14, 15]
    assert QR.quota_walk(scores, order, keys, [10], ids, 6, 2)[2] == [11, 12, 14, 15]      # the seen best neither counts nor fills: the third is promoted
    assert QR.quota_walk(scores, order, keys, [10, 11], ids, 6, 2)[2] == [12, 13, 14, 15]
    assert QR.quota_walk(scores, order, keys, [10, 11, 12], ids, 6, 2)[2] == [13, 14, 15]
    masked = scores.clone()
    masked[1] = NEG_INF
    assert QR.quota_walk(masked, CR.key_order(masked), keys, None, ids, 6, 2)[2] == [10, 12, 14, 15]
    assert QR.quota_topk(scores.reshape(1, -1), keys, None, ids, 5, 2) is None                 # four survivors: the call raises
    got = QR.quota_topk(scores.reshape(1, -1), keys, None, ids, 4, 2)
    assert got[1].tolist() == [[10, 11, 14, 15]] and got[0].tolist() == [[9.0, 8.0, 5.0, 4.0]]


@pytest.mark.parametrize("groups_kind", ["G = 1", "G = N", "groups of ~5"])
def test_round_table_model_is_the_reference(groups_kind):
    """The fallback's argument on the host: the t-th best of every group, side by side, ranked by key = the first k survivors of the walk."""
    g = torch.Generator().manual_seed(103)
    rows, n = 3, 700
    ranks = {"G = 1": torch.zeros(n, dtype=torch.int32), "G = N": torch.randperm(n, generator=g).to(torch.int32),
             "groups of ~5": torch.randint(0, n // 5, (n,), generator=g).to(torch.int32)}[groups_kind]
    groups = int(ranks.max()) + 1
    ids = torch.randperm(n, generator=g) * 3 + 1
    scores = torch.randint(-3, 4, (rows, n), generator=g).float()
    scores[:, torch.randperm(n, generator=g)[:60]] = NEG_INF
    scores[2] = 1.5                                                             # a row where only the position rule decides
    invalid = ids[torch.randint(0, n, (rows, 40), generator=g)]
    for m in (1, 2, 3, 8):
        for inv in (None, invalid):
            table = QR.round_table(scores, ranks, groups, m, ids, inv)
            assert table.shape == (rows, m, groups)
            live = table != 0
            assert bool((live[:, 1:] <= live[:, :-1]).all()) and bool((table[:, 1:][live[:, 1:]] < table[:, :-1][live[:, 1:]]).all())      # rounds descend, 0 after the last
            for k in (1, 10, 200):
                picked = QR.table_topk(table, k)
                for b in range(rows):
                    ws, wp, _ = QR.quota_walk(scores[b], CR.key_order(scores[b]), ranks, None if inv is None else inv[b], ids, k, m)
                    assert picked[b][1] == wp and picked[b][0] == ws, (groups_kind, m, k, b)


def test_int_keys_order_as_key_order():
    scores = torch.tensor([[0.0, -0.0, 1.0, -1.0, 1.0, float("inf"), NEG_INF, 3e-40, -3e-40]])
    keys = QR.int_keys(scores)[0]
    assert np.argsort(keys, kind="stable")[::-1].tolist() == CR.key_order(scores[0]).tolist()


def header_text():
    with open(os.path.join(ROOT, "include", "rails_amd.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_new_entry_points_are_declared_bound_and_exported_under_abi_15():
    header = header_text()
    lib = _lib.load()
    counts = {}
    for name in NEW_ENTRIES + ("rails_topk_collapse", "rails_scores_group_max", "rails_topk_keys"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m is not None, f"{name} is not declared in include/rails_amd.h"
        counts[name] = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.PROTOTYPES, f"{name} is not bound in rails_amd/_lib.py"
        assert len(_lib.PROTOTYPES[name][1]) == counts[name], (name, counts[name])
        assert getattr(lib, name) is not None
    assert counts["rails_topk_collapse_quota"] == counts["rails_topk_collapse"] + 1 == 18      # the same arguments plus max_per_group
    assert counts["rails_scores_group_next"] == 15 and counts["rails_scores_group_max"] == 13 and counts["rails_topk_keys"] == 10
    assert re.search(r"#define\s+RAILS_ABI_VERSION\s+15\b", header)
    assert _lib.RAILS_ABI_VERSION == 15 and lib.rails_abi_version() == 15
    assert E.COLLAPSE_MAX_PER_GROUP == 32 and E.COLLAPSE_MAX_K == 512 and E.COLLAPSE_MAX_SEEN == 4096


def test_new_entry_points_validate_before_any_launch():
    """No device is needed: every refused call returns before it would launch.  (1 stands for a non-NULL pointer; nothing dereferences it.)"""
    lib = _lib.load()
    bad, ok = _lib.RAILS_EINVAL, _lib.RAILS_OK
    # rails_topk_collapse_quota(scores, ld, positions, rows, depth, group_ranks, n_items, ids, invalid_ids, width, k, max_per_group, out_scores,
    #                           out_positions, out_ids, out_counts, out_of_range, stream)
    good = [1, 8, 1, 2, 8, 1, 100, None, None, 0, 3, 2, 1, 1, 1, 1, 1]
    for m in (0, -1):
        args = list(good)
        args[11] = m
        assert lib.rails_topk_collapse_quota(*args, None) == bad and "max_per_group" in _lib.last_error()
    for at in (0, 2, 5, 12, 13, 14, 15, 16):
        args = list(good)
        args[at] = None
        assert lib.rails_topk_collapse_quota(*args, None) == bad and "NULL" in _lib.last_error(), at
    args = list(good)
    args[1] = 7
    assert lib.rails_topk_collapse_quota(*args, None) == bad and "ld < depth" in _lib.last_error()
    for depth in (0, 16385):
        args = list(good)
        args[1], args[4] = depth, depth
        assert lib.rails_topk_collapse_quota(*args, None) == _lib.RAILS_ENOTSUP and "depth" in _lib.last_error()
    args = list(good)
    args[3] = 0
    assert lib.rails_topk_collapse_quota(*args, None) == ok
    # rails_scores_group_next(scores, ld, rows, n, first_item, group_ranks, n_groups, table, table_stride, below, below_stride, ids, invalid_ids,
    #                         width, stream)
    good = [1, 10, 2, 10, 0, 1, 4, 16, 8, 8, 8, None, None, 0]
    for at in (0, 5, 7):
        args = list(good)
        args[at] = None
        assert lib.rails_scores_group_next(*args, None) == bad and "NULL" in _lib.last_error(), at
    for at, value, word in ((1, 9, "ld < n"), (8, 3, "stride"), (10, 3, "stride"), (9, 16, "bound itself"), (2, -1, "negative"), (4, -1, "negative")):
        args = list(good)
        args[at] = value
        assert lib.rails_scores_group_next(*args, None) == bad and word in _lib.last_error(), (at, _lib.last_error())
    for at, value in ((13, 4097), (4, (1 << 32) - 5), (2, 65536)):
        args = list(good)
        args[at] = value
        if at == 13:
            args[12] = 1
        assert lib.rails_scores_group_next(*args, None) == _lib.RAILS_ENOTSUP, at
    for at in (2, 3, 6):      # nothing to do
        args = list(good)
        args[at] = 0
        if at == 6:
            args[8] = args[10] = 0
        assert lib.rails_scores_group_next(*args, None) == ok, at


# ---- argument checks and refusals: message by message, on modules that are never launched ---------------------------------------------------
class Exact(T.MIPSBruteForceTopK):
    """_take_collapse and the checks of _collapsed_exact read the type, the group row, k, m and the seen ids' width: no index is needed."""

    def __init__(self, groups=True):
        torch.nn.Module.__init__(self)
        self._groups = torch.tensor([0, 0, 1, -1], dtype=torch.int32) if groups else None


def test_take_collapse_returns_m():
    tk = Exact()
    for kwargs, want in (({}, 0), ({"collapse_groups": False}, 0), ({"collapse_groups": True}, 1), ({"max_per_group": 1}, 1),
                         ({"max_per_group": 3}, 3), ({"collapse_groups": False, "max_per_group": 4}, 4), ({"collapse_groups": True, "max_per_group": 1}, 1),
                         ({"max_per_group": 1000}, 1000), ({"collapse_groups": False, "max_per_group": None}, 0)):
        kw = dict(kwargs, user_ids=7)
        assert T._asks_collapse(kw) == bool(kwargs)
        assert tk._take_collapse(kw) == want and kw == {"user_ids": 7}, kwargs      # both arguments are taken out of the call
    assert tk.collapse_stats() == {"calls": 0, "walk_redos": 0, "fallbacks": 0}


def test_argument_checks():
    tk = Exact()
    for m in (0, -2, True, False, 2.0, "2", torch.tensor(2), np.int64(2)):
        with pytest.raises(ValueError) as e:
            tk._take_collapse({"max_per_group": m})
        assert str(e.value) == f"Exact: max_per_group must be a Python int >= 1, got {m!r}"
    for m in (2, 7):
        with pytest.raises(ValueError) as e:
            tk._take_collapse({"collapse_groups": True, "max_per_group": m})
        assert str(e.value) == f"Exact: collapse_groups=True means max_per_group=1, got max_per_group={m} with it (pass one of the two)"
    bare = Exact(groups=False)
    with pytest.raises(ValueError) as e:
        bare._take_collapse({"max_per_group": 2})
    assert str(e.value) == "Exact: max_per_group=2 on a module without groups (set_item_groups first)"
    with pytest.raises(ValueError) as e:
        bare._take_collapse({"collapse_groups": True})
    assert str(e.value) == "Exact: collapse_groups=True on a module without groups (set_item_groups first)"      # (as it is today)
    # through the public calls: the checks come first, nothing of the (absent) index is touched
    q = torch.zeros(2, 4)
    for call in (lambda **kw: tk.forward(q, 3, **kw), lambda **kw: tk.forward_filtered(q, 3, torch.zeros((2, 1), dtype=torch.int64), 3, **kw)):
        with pytest.raises(ValueError, match="Python int"):
            call(max_per_group=0)
        with pytest.raises(ValueError, match="means max_per_group=1"):
            call(max_per_group=2, collapse_groups=True)


def test_limits_of_the_exact_modules_come_before_any_launch():
    tk, q = Exact(), torch.zeros(2, 4)
    with pytest.raises(NotImplementedError) as e:
        tk.forward(q, 513, max_per_group=2)
    assert str(e.value) == ("Exact: max_per_group=2 takes k <= 512 and up to 4096 seen ids per row (what its exact group-maxima pass selects and "
                            "filters), got k = 513, width = 0")
    with pytest.raises(NotImplementedError) as e:
        tk.forward(q, 513, collapse_groups=True)
    assert str(e.value) == ("Exact: collapse_groups=True takes k <= 512 and up to 4096 seen ids per row (what its exact group-maxima pass selects and "
                            "filters), got k = 513, width = 0")      # (as it is today)
    with pytest.raises(NotImplementedError) as e:
        tk.forward_filtered(q, 3, torch.zeros((2, 4097), dtype=torch.int64), 3, max_per_group=2)
    assert str(e.value).startswith("Exact: max_per_group=2 takes k <= 512") and str(e.value).endswith("got k = 3, width = 4097")
    for k, m in ((40, 33), (33, 1000), (512, 40)):      # the limit is on m_eff = min(m, k)
        with pytest.raises(NotImplementedError) as e:
            tk.forward(q, k, max_per_group=m)
        assert str(e.value) == ("Exact: max_per_group takes min(max_per_group, k) <= 32 on the exact modules (their fallback reads the scores once per "
                                f"result of a group), got {min(m, k)}")
    tk.MAX_LOGIT_BYTES = 3 * 3 * 8 - 1      # three ranks (0, 1 and the ungrouped item's own), m_eff = 3: one row of the table does not fit
    with pytest.raises(NotImplementedError) as e:
        tk.forward(q, 3, max_per_group=5)
    assert str(e.value) == "Exact: max_per_group=3 needs 72 bytes of group keys per query for its exact fallback, beyond MAX_LOGIT_BYTES = 71"
    assert tk.collapse_stats() == {"calls": 0, "walk_redos": 0, "fallbacks": 0}


def test_refusals_by_name():
    class Wrapper:
        pass

    w = Wrapper()
    T.refuse_collapse_groups(w, {})
    T.refuse_collapse_groups(w, {"collapse_groups": False, "max_per_group": None})
    with pytest.raises(NotImplementedError) as e:
        T.refuse_collapse_groups(w, {"max_per_group": 2})
    assert str(e.value) == ("Wrapper takes no max_per_group: a quota per item group is built on the single-device modules' forward, forward_filtered, "
                            "submit and get_top_k_outputs only")
    with pytest.raises(NotImplementedError) as e:
        T.refuse_collapse_groups(w, {"max_per_group": 1}, "all_logits")
    assert str(e.value).startswith("Wrapper.all_logits takes no max_per_group: ")
    with pytest.raises(NotImplementedError) as e:
        T.refuse_collapse_groups(w, {"collapse_groups": True}, "topk_ids")
    assert str(e.value) == ("Wrapper.topk_ids takes no collapse_groups: collapsing by item group is built on the single-device modules' forward, "
                            "forward_filtered, submit and get_top_k_outputs only")      # (as it is today)
    with pytest.raises(NotImplementedError) as e:
        T.refuse_collapse_groups(w, {"collapse_groups": True, "max_per_group": 2})
    assert " takes no collapse_groups: " in str(e.value)
    # the streaming family's entry check, on an exact module: after the family's own refusal, before anything else
    tk = Exact()
    for what in ("rank_of", "log_partition", "range_search"):
        with pytest.raises(NotImplementedError) as e:
            tk._refuse_streaming({"max_per_group": 2}, what, None)
        assert str(e.value).startswith(f"Exact.{what} takes no max_per_group: ")
        with pytest.raises(NotImplementedError) as e:
            tk._refuse_streaming({"collapse_groups": True}, what, None)
        assert str(e.value).startswith(f"Exact.{what} takes no collapse_groups: ")
    # the IVF module and the approximate modules of the generic route refuse by the argument's own name
    ivf = types.SimpleNamespace(_use_faiss=True, _call_eng=None, _engine=types.SimpleNamespace(route="fp32"))
    for what in ("max_per_group", "collapse_groups"):
        with pytest.raises(NotImplementedError) as e:
            T.MoLNaiveTopK._check_collapsible(ivf, what)
        assert str(e.value) == (f"MoLNaiveTopK (IVF, use_faiss=True) takes no {what}: collapsing by item group is not built on the IVF index; the "
                                "exhaustive MoLNaiveTopK takes it")
    generic = types.SimpleNamespace(_use_faiss=False, _call_eng=None, _engine=types.SimpleNamespace(route="generic"))
    for cls in (T.MoLNaiveTopK, T.MoLAvgTopK):
        with pytest.raises(NotImplementedError) as e:
            cls._check_collapsible(generic, "max_per_group")
        assert str(e.value) == ("SimpleNamespace: max_per_group is not built on the generic scoring route (generic_candidates = True covers the "
                                "single-device exhaustive algorithms without item groups); MoLBruteForceTopK collapses by item group on this route")


def test_sharded_wrappers_refuse_by_name():
    from rails_amd import sharded

    class OneRank(sharded.ShardedMoLAvgTopK):
        def __init__(self):      # (no process group: the refusal comes before anything of the wrapper is touched)
            torch.nn.Module.__init__(self)

    q = torch.zeros(2, 4)
    for call in (lambda w: w.forward(q, 3, max_per_group=2), lambda w: w.forward_filtered(q, 4, torch.zeros((2, 1), dtype=torch.int64), 3, max_per_group=2)):
        with pytest.raises(NotImplementedError, match="OneRank takes no max_per_group"):
            call(OneRank())


def test_kernel_resources():
    """The code-object metadata of the built kernels (tools/kernel_resources.sh): neither new kernel spills, and the walk with a quota holds
    exactly the static LDS of the plain walk -- its dynamic LDS is the same launch formula (147 456 bytes at depth 16 384), so the quota may
    add nothing per entry."""
    import subprocess

    llvm = "/opt/rocm/lib/llvm/bin"
    # (no skip: the library this suite runs was built from these objects by build(), with these tools; a tree without them is not checked)
    assert os.path.exists(os.path.join(llvm, "llvm-readelf")) and os.path.exists(os.path.join(llvm, "clang-offload-bundler")), "LLVM tools of ROCm not found"
    assert os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "collapse.o")), "objects not built (python -c 'import __graft_entry__ as g; g.build()')"
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "collapse_walk_kernel|group_next_kernel"],
                         capture_output=True, text=True, timeout=600).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"vgpr\s+(\d+) agpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+)\s+(.*)$", line.strip())
        if m:
            name = re.search(r"(\w+(?:<\w+>)?)\(", m.group(6)).group(1)
            rows[name] = {"vgpr": int(m.group(1)), "scratch": int(m.group(4)), "lds": int(m.group(5))}
    table = {"collapse_walk_kernel<true>": 128, "collapse_walk_kernel<false>": 128, "group_next_kernel": 64}      # VGPR ceilings
    assert sorted(rows) == sorted(table), out[-2000:]
    for name, vgpr in table.items():
        assert rows[name]["scratch"] == 0 and rows[name]["vgpr"] <= vgpr, (name, rows[name])
    assert rows["collapse_walk_kernel<true>"]["lds"] == rows["collapse_walk_kernel<false>"]["lds"]
    assert rows["group_next_kernel"]["lds"] == 0      # (the seen ids are dynamic LDS)
    src = open(os.path.join(ROOT, "rails_amd", "csrc", "collapse.hip")).read()
    assert "block_scan_max_excl<kCollapseThreads>" in src and "collapse_walk_kernel<true>" in src and "collapse_walk_kernel<false>" in src
