"""GPU: rank_of.  The kernels of rails_amd/csrc/rank.hip against tests/_rank_ref.py, exact equality; the contract of
rank_of on MoLBruteForceTopK (every exact_mode, precision and route) and MIPSBruteForceTopK -- rank - 1 is the target's index in the row's
exhaustive get_top_k_outputs list, over exactly the items the row may return --; the eval harness's exact_ranks switch against its default path.
Inputs and helpers: those of tests/test_item_mask_gpu.py and tests/test_index_update_gpu.py."""
import numpy as np
import pytest
import torch

import rails_amd
from rails_amd import engine as E
from tests import _rank_ref
from tests import _topk_ref as R
from tests import test_index_update_gpu as U
from tests import test_item_mask_gpu as M
from tests.test_index_update_gpu import B
from tests.test_item_mask_gpu import N, SIZES

pytestmark = pytest.mark.gpu
ROWS = 3
FAMILY_NAMES = ("gauss", "constant", "signed_zeros", "nans", "all_negative", "subnormals", "infs")
TS = (1, 2, 5, 64, 70)
PAD_BITS = 0x7FC0FFEE      # what lies between the rows of a matrix with ld > n: a NaN that would outrank everything if it were read


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def family_rows(name, n, rng):
    """(ROWS, n) uint32 score bit patterns"""
    rows = np.stack([R.FAMILIES["gauss" if name == "infs" else name](n, max(1, n // 2), rng) for _ in range(ROWS)])
    if name == "infs":
        for r in range(ROWS):
            where = rng.permutation(n)[:4]
            rows[r, where[0::2]] = 0x7F800000
            rows[r, where[1::2]] = 0xFF800000
            rows[r, n - 1] = 0xFF800000 if r % 2 else 0x7F800000
    return rows


def on_device(bits, ld, lead, dev):
    """The rows as an (rows, n) fp32 view with row stride ld whose first element sits `lead` elements past an aligned address"""
    rows, n = bits.shape
    buf = np.full(lead + rows * ld, PAD_BITS, dtype=np.uint32)
    for r in range(rows):
        buf[lead + r * ld : lead + r * ld + n] = bits[r]
    flat = torch.from_numpy(buf.view(np.int32)).to(dev).view(torch.float32)
    return flat[lead:].as_strided((rows, n), (ld, 1))


def targets_for(bits, eligible, t, shift, rng):
    """(ROWS, t) int64: a window of t out of -- positions 0, n - 1, 31 and 32, the row's best and worst eligible item, a cleared position, -1,
    one position twice -- and random ones"""
    rows, n = bits.shape
    out = np.zeros((rows, t), dtype=np.int64)
    for r in range(rows):
        kv = R.keys(bits[r])
        kept, gone = np.nonzero(eligible[r])[0], np.nonzero(~eligible[r])[0]
        best = kept[np.argmax(kv[kept])] if kept.size else 0
        worst = kept[np.argmin(kv[kept])] if kept.size else n - 1
        twice = int(rng.integers(0, n))
        special = [0, n - 1, 31, 32, best, worst, gone[rng.integers(0, gone.size)] if gone.size else -1, -1, twice, twice]
        pool = np.concatenate([np.roll(np.array(special, dtype=np.int64), -shift), rng.integers(0, n, size=max(0, t - len(special)))])
        out[r] = pool[:t]
    return out


def kernel_cases(n, rng):
    """(what, eligible (ROWS, n) bool, mask argument maker) for no mask and every pattern, shared and per row"""
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    yield "no mask", np.ones((ROWS, n), dtype=bool), lambda dev: None
    for name, mask in M.patterns(ROWS, n, g).items():
        yield f"{name}, shared", mask[:1].expand(ROWS, n).numpy(), (lambda dev, m=mask: E.ItemMask(m[0].to(dev)))
        yield f"{name}, per row", mask.numpy(), (lambda dev, m=mask: E.ItemMask(m.to(dev)))


@pytest.mark.parametrize("extra_ld", [0, 5])
def test_scores_rank_against_the_reference(extra_ld, dev):
    rng = np.random.default_rng(40 + extra_ld)
    case = 0
    seen = set()
    for n in SIZES:
        for what, eligible, make_mask in kernel_cases(n, rng):
            fam, t = FAMILY_NAMES[case % len(FAMILY_NAMES)], TS[(case // 3) % len(TS)]
            bits = family_rows(fam, n, rng)
            targets = targets_for(bits, eligible, t, case % 10, rng)
            want = _rank_ref.ranks(bits, eligible, targets)
            scores = on_device(bits, n + extra_ld, 3 if extra_ld else 0, dev)
            got = E.scores_rank(scores, torch.from_numpy(targets).to(dev), make_mask(dev))
            assert got.dtype == torch.int64 and got.shape == (ROWS, t)
            assert np.array_equal(got.cpu().numpy(), want), f"n = {n}, ld = n + {extra_ld}, t = {t}, {fam}, {what}"
            seen.add((fam, t))
            case += 1
    assert {f for f, _ in seen} == set(FAMILY_NAMES) and {t for _, t in seen} == set(TS)


def test_scores_rank_special_targets(dev):
    """What the special targets must give, stated on its own: best -> 1, worst -> the kept count, a cleared or unknown target -> 0, a position
    given twice -> the same rank twice; the mask handed over as an ItemMask or as its words."""
    rng = np.random.default_rng(43)
    n = 3 * 4096 + 37
    bits = family_rows("gauss", n, rng)
    eligible = rng.random((ROWS, n)) < 0.5
    kv = np.stack([R.keys(bits[r]) for r in range(ROWS)])
    best = [int(np.nonzero(eligible[r])[0][np.argmax(kv[r][eligible[r]])]) for r in range(ROWS)]
    worst = [int(np.nonzero(eligible[r])[0][np.argmin(kv[r][eligible[r]])]) for r in range(ROWS)]
    gone = [int(np.nonzero(~eligible[r])[0][7]) for r in range(ROWS)]
    targets = np.array([[best[r], worst[r], gone[r], -1, n, 77, 77] for r in range(ROWS)], dtype=np.int64)
    mask = E.ItemMask(torch.from_numpy(eligible).to(dev))
    scores = on_device(bits, n + 5, 1, dev)
    for m in (mask, mask.words):
        got = E.scores_rank(scores, torch.from_numpy(targets).to(dev), m).cpu().numpy()
        assert np.array_equal(got, _rank_ref.ranks(bits, eligible, targets))
        for r in range(ROWS):
            assert got[r, :5].tolist() == [1, int(eligible[r].sum()), 0, 0, 0] and got[r, 5] == got[r, 6]
    with pytest.raises(ValueError, match="rows"):
        E.scores_rank(scores[:2], torch.from_numpy(targets[:2]).to(dev), mask)
    with pytest.raises(ValueError, match="positions"):
        E.scores_rank(scores, torch.from_numpy(targets[:2]).to(dev), mask)
    with pytest.raises(ValueError, match="mask of"):
        E.scores_rank(scores[:, : n - 1], torch.from_numpy(targets).to(dev), mask)


def test_scores_rank_many_workgroups_per_counter(dev):
    rng = np.random.default_rng(44)
    n, rows = 300_007, 2
    bits = np.stack([R.FAMILIES["gauss"](n, 1000, rng) for _ in range(rows)])
    bits[1, ::3] = bits[1, 0]      # long runs of ties: the position half of the key decides
    eligible = rng.random((rows, n)) < 0.5
    targets = np.stack([np.concatenate([[0, n - 1, -1], rng.integers(0, n, size=13)]) for _ in range(rows)]).astype(np.int64)
    scores = on_device(bits, n + 1, 0, dev)
    for elig, mask in ((np.ones_like(eligible), None), (eligible, E.ItemMask(torch.from_numpy(eligible).to(dev)))):
        got = E.scores_rank(scores, torch.from_numpy(targets).to(dev), mask)
        assert np.array_equal(got.cpu().numpy(), _rank_ref.ranks(bits, elig, targets))


def test_item_mask_clear_rows_against_numpy(dev):
    rng = np.random.default_rng(45)
    for n in SIZES:
        words = (n + 31) // 32
        stride = words + 3
        start = rng.integers(0, 1 << 32, size=(ROWS, stride), dtype=np.uint64).astype(np.uint32)
        m = int(rng.integers(1, 40))
        pos = rng.integers(0, n, size=(ROWS, m)).astype(np.int64)
        pos[:, m // 2] = pos[:, 0]                     # a repeat
        pos[0, -1], pos[1, -1], pos[2, -1] = -1, n, n - 1
        if m > 3:
            pos[0, 1], pos[1, 1], pos[2, 1] = 0, 31 if n > 31 else 0, 32 if n > 32 else n + 7
        want = start.copy()
        for r in range(ROWS):
            for p in pos[r]:
                if 0 <= p < n:
                    want[r, p >> 5] &= ~np.uint32(1 << (p & 31))
        d = torch.from_numpy(start.view(np.int32)).to(dev)
        view = d[:, :words] if n % 2 else d            # rows of `words` words with stride words + 3, or the whole rows
        out = E.item_mask_clear_rows(view, torch.from_numpy(pos).to(dev), n)
        assert out.data_ptr() == d.data_ptr()
        assert np.array_equal(d.cpu().numpy().view(np.uint32), want), n
    with pytest.raises(ValueError, match="do not hold"):
        E.item_mask_clear_rows(torch.zeros((2, 3), dtype=torch.int32, device=dev), torch.zeros((2, 1), dtype=torch.int64, device=dev), 97)
    with pytest.raises(ValueError, match="positions"):
        E.item_mask_clear_rows(torch.zeros((2, 3), dtype=torch.int32, device=dev), torch.zeros((3, 1), dtype=torch.int64, device=dev))


# ---- the module contract -----------------------------------------------------------------------------------------------------------------
ROUTES = [("brute", r) for r in ("default", "dense", "f16x3", "c4", "generic")] + [("mips", "mips")]


def logit_bits(tk, q, aux):
    """The module's own all_logits bits (MIPSBruteForceTopK has no all_logits: the score matrix its forward selects from) -> (B, N) uint32"""
    logits = tk.all_logits(q, **aux) if hasattr(tk, "all_logits") else tk._index.score(q)
    return logits.view(torch.int32).cpu().numpy().view(np.uint32)


def ref_ranks(bits, eligible, target_pos):
    eligible = np.broadcast_to(eligible, bits.shape)
    return torch.from_numpy(_rank_ref.ranks(bits, eligible, target_pos.cpu().numpy()))


def random_targets(g, t=5):
    return torch.randint(0, N, (B, t), generator=g)


@pytest.mark.parametrize("module,route", ROUTES)
def test_rank_of_is_the_index_in_the_exhaustive_list(module, route, dev):
    make, X, ids, q, aux = M.setup(module, route, dev)
    g = torch.Generator().manual_seed(51)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        bits = logit_bits(tk, q, aux)
        # (a) random targets, by id and by position, against the reference over the module's own logits
        pos = random_targets(g)
        want = ref_ranks(bits, np.ones((1, N), dtype=bool), pos)
        got = tk.rank_of(q, ids[pos.to(dev)], **aux)
        assert got.dtype == torch.int64 and got.shape == (B, 5) and got.device == q.device
        assert torch.equal(got.cpu(), want) and int(want.min()) >= 1, f"{module} {route}: rank_of"
        assert torch.equal(tk.rank_of_positions(q, pos.to(dev), **aux).cpu(), want), f"{module} {route}: rank_of_positions"
        unknown = ids[pos.to(dev)].clone()
        unknown[:, 2] = 2                                                # (ids are 3 * position + 1)
        want[:, 2] = 0
        assert torch.equal(tk.rank_of(q, unknown, **aux).cpu(), want), f"{module} {route}: an id nobody has"
        # (b) the ids forward returns stand where it put them
        scores200, ids200 = tk(q, k=200, **aux)
        at = torch.tensor([0, 1, 119, 199], device=dev)
        assert torch.equal(tk.rank_of(q, ids200[:, at].contiguous(), **aux).cpu(), (at + 1).cpu().expand(B, -1)), f"{module} {route}: forward's ids"
        # (c) seen ids leave the row's eligible set: they rank 0, and the filtered top-50 ranks 1 .. 50
        seen = torch.cat([ids200[:, 5:66], torch.tensor([[2, 5]], device=dev).expand(B, -1)], dim=1).contiguous()
        assert torch.equal(tk.rank_of(q, ids200[:, 5:66].contiguous(), invalid_ids=seen, **aux), torch.zeros((B, 61), dtype=torch.int64, device=dev))
        cand = rails_amd.CandidateIndex(ids=ids.reshape(1, -1), embeddings=X.unsqueeze(0))
        top50 = cand.get_top_k_outputs(q, 50, aux, tk, seen)[0]
        assert torch.equal(tk.rank_of(q, top50, invalid_ids=seen, **aux).cpu(), torch.arange(1, 51).expand(B, -1)), f"{module} {route}: filtered top-50"
        elig = np.ones((B, N), dtype=bool)
        np.put_along_axis(elig, ((ids200[:, 5:66] - 1) // 3).cpu().numpy(), False, axis=1)
        assert torch.equal(tk.rank_of_positions(q, pos.to(dev), invalid_ids=seen, **aux).cpu(), ref_ranks(bits, elig, pos)), f"{module} {route}: seen ids"
        # (f) three batch slices under the logit policy give the unsliced result
        whole = tk.rank_of_positions(q, pos.to(dev), invalid_ids=seen, **aux)
        tk.MAX_LOGIT_BYTES = 11 * N * 4
        assert torch.equal(tk.rank_of_positions(q, pos.to(dev), invalid_ids=seen, **aux), whole), f"{module} {route}: sliced"
        tk.MAX_LOGIT_BYTES = N * 4 - 1
        with pytest.raises(NotImplementedError, match=type(tk).__name__ + r"\.rank_of: one row"):
            tk.rank_of_positions(q, pos.to(dev), **aux)


@pytest.mark.parametrize("module,route", ROUTES)
def test_rank_of_honours_what_a_row_may_return(module, route, dev):
    """(d) a hidden set, per-row allowed_tags= and a ragged per-row item_mask=; a shared restriction also against a fresh module of the kept items."""
    make, X, ids, q, aux = M.setup(module, route, dev)
    g = torch.Generator().manual_seed(52)
    with torch.inference_mode():
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        bits = logit_bits(tk, q, aux)
        best = ((tk(q, k=10, **aux)[1][:8, :2] - 1) // 3).reshape(-1).cpu()
        pos = torch.cat([random_targets(g, 4), ((tk(q, k=10, **aux)[1][:, :1] - 1) // 3).cpu()], dim=1)       # ... and each row's own best item
        target_ids = ids[pos.to(dev)]
        hidden = torch.unique(torch.cat([best, torch.randperm(N, generator=g)[:5000], torch.tensor([0, 31, 32, N - 1])]))
        vis = torch.ones(N, dtype=torch.bool)
        vis[hidden] = False
        m60 = torch.rand(N, generator=g) < 0.6
        r200 = torch.zeros(N, dtype=torch.bool)
        r200[torch.randperm(N, generator=g)[:200]] = True
        three = [torch.ones(N, dtype=torch.bool), torch.rand(N, generator=g) < 0.5, r200]
        per_row = torch.stack([three[b % 3] for b in range(B)])
        per_row[torch.arange(B), pos[:, 1]] = True                       # (one target of every row is inside its mask)
        tags = torch.randint(0, 8, (N,), generator=g)
        allowed = [(1, 2, 5)[b % 3] for b in range(B)]

        def fresh_of(keep):
            f = make(X[keep.to(dev)].clone().unsqueeze(0), ids[keep.to(dev)].clone().unsqueeze(0))
            return f.rank_of(q, target_ids, **aux)

        # a shared item_mask= on a module without a hidden set
        got = tk.rank_of(q, target_ids, item_mask=E.ItemMask(m60.to(dev)), **aux)
        assert torch.equal(got.cpu(), ref_ranks(bits, m60.numpy()[None], pos)), f"{module} {route}: shared mask"
        assert torch.equal(got, fresh_of(m60)), f"{module} {route}: shared mask, fresh module"
        # the hidden set alone, then under a mask, a ragged per-row mask and per-row tags
        tk.hide_items(hidden)
        got = tk.rank_of(q, target_ids, **aux)
        assert torch.equal(got.cpu(), ref_ranks(bits, vis.numpy()[None], pos)), f"{module} {route}: hidden set"
        assert torch.equal(got, fresh_of(vis)) and int((got == 0).sum()) >= 8, f"{module} {route}: hidden set, fresh module"
        got = tk.rank_of(q, target_ids, item_mask=m60.to(dev), **aux)
        assert torch.equal(got.cpu(), ref_ranks(bits, (m60 & vis).numpy()[None], pos)), f"{module} {route}: hidden set and shared mask"
        assert torch.equal(got, fresh_of(m60 & vis))
        got = tk.rank_of(q, target_ids, item_mask=E.ItemMask(per_row.to(dev)), **aux)
        assert torch.equal(got.cpu(), ref_ranks(bits, (per_row & vis[None]).numpy(), pos)), f"{module} {route}: ragged per-row mask"
        seen = ids[pos[:, 3:4].to(dev)].contiguous()                     # ... and with one target of every row seen
        elig = (per_row & vis[None]).clone()
        elig[torch.arange(B), pos[:, 3]] = False
        got = tk.rank_of(q, target_ids, invalid_ids=seen, item_mask=E.ItemMask(per_row.to(dev)), **aux)
        assert torch.equal(got.cpu(), ref_ranks(bits, elig.numpy(), pos)) and not bool(got[:, 3].any()), f"{module} {route}: per-row mask and seen ids"
        tk.set_item_tags(tags.to(dev))
        by_tag = (tags[None, :] & torch.tensor(allowed)[:, None]) != 0
        got = tk.rank_of(q, target_ids, allowed_tags=allowed, **aux)
        assert torch.equal(got.cpu(), ref_ranks(bits, (by_tag & vis[None]).numpy(), pos)), f"{module} {route}: per-row allowed_tags"
        got = tk.rank_of(q, target_ids, allowed_tags=5, **aux)
        assert torch.equal(got, fresh_of(((tags & 5) != 0) & vis)), f"{module} {route}: shared allowed_tags, fresh module"
        with pytest.raises(ValueError, match="allowed_tags= and item_mask="):
            tk.rank_of(q, target_ids, allowed_tags=5, item_mask=m60.to(dev), **aux)


@pytest.mark.parametrize("module,route", ROUTES)
def test_rank_of_on_an_all_tie_corpus(module, route, dev):
    """(e) every item row identical: every score of a row is the same bits, and the position half of the key ranks alone."""
    make, X, ids, q, aux = M.setup(module, route, dev)
    g = torch.Generator().manual_seed(53)
    with torch.inference_mode():
        tk = make(X[:1].expand(N, -1).contiguous().unsqueeze(0), ids.unsqueeze(0))
        bits = logit_bits(tk, q, aux)
        assert (bits == bits[:, :1]).all(), "the scores of identical items differ"
        pos = torch.cat([random_targets(g, 4), torch.tensor([[0, 31, 32, N - 1]]).expand(B, -1)], dim=1)
        assert torch.equal(tk.rank_of_positions(q, pos.to(dev), **aux).cpu(), pos + 1)
        keep = torch.rand(N, generator=g) < 0.5
        below = torch.cumsum(keep, 0) - keep.long()                       # eligible positions below each position
        want = torch.where(keep[pos], below[pos] + 1, torch.zeros_like(pos))
        assert torch.equal(tk.rank_of_positions(q, pos.to(dev), item_mask=keep.to(dev), **aux).cpu(), want)


@pytest.mark.parametrize("module,route", ROUTES)
def test_rank_of_after_corpus_edits(module, route, dev):
    """(g) update_items / append_items / remove_items, with the id map live: the answers of a module freshly built from the resulting corpus."""
    from tests import test_index_remove_gpu as RM

    make, X, ids, q, aux = M.setup(module, route, dev)
    cfg = U.O.CONFIGS["amzn-books"] if module == "mips" else U.setup_route(module, route, dev)[0]
    g = torch.Generator().manual_seed(54)
    with torch.inference_mode():
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        top = tk(q, k=10, **aux)[1]
        target_ids = torch.cat([top[:, :3], ids[random_targets(g, 3).to(dev)], torch.tensor([[-7, -8]], device=dev).expand(B, -1)], dim=1).contiguous()
        first = tk.rank_of(q, target_ids, **aux)                          # (the id map exists from here on)
        assert torch.equal(first[:, :3].cpu(), torch.arange(1, 4).expand(B, -1)) and not bool(first[:, 6:].any())
        X2, ids2 = X.clone(), ids.clone()
        upd = U.positions_for(N, g)
        rows = U.table(cfg, upd.numel(), 31, dev, first=20_000_000)
        tk.update_items(upd, rows)
        X2[upd.to(dev)] = rows
        extra = U.table(cfg, 70, 32, dev, first=30_000_000)
        extra[:2] = X[((top[:2, 0] - 1) // 3)]                            # copies of two queries' best items: the appended rows enter the head
        new_ids = torch.tensor([-7, -8], device=dev).new_tensor(list(range(-7, -77, -1)))
        tk.append_items(extra, new_ids)
        X2, ids2 = torch.cat([X2, extra]), torch.cat([ids2, new_ids])
        gone = RM.removal_set(N + 70, g, must=((top[:4, 1] - 1) // 3).cpu())
        tk.remove_items(gone)
        X2, ids2, _ = RM.after_removal(X2, ids2, gone)
        fresh = make(X2.clone().unsqueeze(0), ids2.clone().unsqueeze(0))
        seen = top[:, 3:9].contiguous()
        for kw in ({}, {"invalid_ids": seen}):
            got, want = tk.rank_of(q, target_ids, **kw, **aux), fresh.rank_of(q, target_ids, **kw, **aux)
            assert torch.equal(got, want), f"{module} {route}: after the edits {sorted(kw)}"
        assert not torch.equal(got, first) and bool((got[:4, 1] == 0).all())      # (removed targets are unknown now)
        bits = logit_bits(fresh, q, aux)
        pos = fresh.positions_of(target_ids.reshape(-1)).view(B, -1)
        assert torch.equal(tk.rank_of(q, target_ids, **aux).cpu(), ref_ranks(bits, np.ones((1, bits.shape[1]), dtype=bool), pos))


def test_refusals(dev):
    """(h) by name: the approximate modules, collapse_groups=True, malformed arguments."""
    cfg, mol, make, aux = U.setup_route("brute", "default", dev)
    n = 20_000
    with torch.inference_mode():
        X, ids = U.table(cfg, n, 16, dev), U.ids_of(n, dev)
        q = U.O.synthetic_queries(cfg, B, seed=11).to(dev)
        t = ids[:B].reshape(B, 1).contiguous()
        others = {"avg": U.MAKERS["avg"](mol, X.unsqueeze(0), ids.unsqueeze(0)), "naive": U.MAKERS["naive"](mol, X.unsqueeze(0), ids.unsqueeze(0)),
                  "comb": U.MAKERS["comb"](mol, X.unsqueeze(0), ids.unsqueeze(0)),
                  "ivf": rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids.unsqueeze(0), k_per_group=5, use_faiss=True)}
        for name, other in others.items():
            for call in (other.rank_of, other.rank_of_positions):
                with pytest.raises(NotImplementedError, match=type(other).__name__ + r"\.rank_of.*MoLBruteForceTopK"):
                    call(q, t)
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        with pytest.raises(NotImplementedError, match=r"MoLBruteForceTopK\.rank_of takes no collapse_groups"):
            tk.rank_of(q, t, collapse_groups=True)
        for wrong in (t[:5], t.reshape(-1), t.float()):
            with pytest.raises(ValueError, match="target_ids"):
                tk.rank_of(q, wrong)
        with pytest.raises(ValueError, match="positions"):
            tk.rank_of_positions(q, t.to(torch.int32))
        with pytest.raises(ValueError, match="invalid_ids"):
            tk.rank_of(q, t, invalid_ids=t[:5])
        with pytest.raises(ValueError, match="rows"):
            tk.rank_of(q, t, item_mask=torch.ones((5, n), dtype=torch.bool, device=dev))
        doubled = rails_amd.MoLBruteForceTopK(mol, X.unsqueeze(0), torch.cat([ids[:1], ids[:-1]]).unsqueeze(0))
        with pytest.raises(ValueError, match="cannot be addressed by id"):      # the id map's refusal of a corpus with repeated ids
            doubled.rank_of(q, t)
        assert torch.equal(doubled.rank_of_positions(q, torch.zeros((B, 1), dtype=torch.int64, device=dev)) >= 1, torch.ones((B, 1), dtype=torch.bool, device=dev))


# ---- the eval harness ------------------------------------------------------------------------------------------------------------------
def test_eval_harness_exact_ranks_against_the_default_path(dev):
    from rails_amd import eval_harness as H
    from tests.test_gpu_parity import Fixture, build_module

    fx = Fixture("harness")
    mol = build_module(fx.cfg, fx.weights, dev)
    X, ids, q = fx.t("X").to(dev), fx.t("item_ids"), fx.t("q").to(dev)
    past, target = fx.t("past_ids").to(dev), fx.t("target_ids").to(dev)
    id_to_row = {int(v): j for j, v in enumerate(ids.view(-1).tolist())}

    class StubEncoder:                       # the query encoder is upstream of the path: replay its output
        def encode(self, **kw):
            return q

        def get_item_embeddings(self, item_ids):
            rows = torch.tensor([id_to_row.get(int(v), 0) for v in item_ids.reshape(-1).tolist()], device=dev)
            return X[0][rows].reshape(item_ids.shape + (X.shape[-1],))

    model = StubEncoder()
    holder = type("M", (), {"_ndp_module": mol})()
    state = H.get_eval_state(model, ids.view(-1).tolist(), None, lambda e, i: rails_amd.get_top_k_module("MoLBruteForceTopK", holder, e, i), dev)
    n_items = state.candidate_index.num_objects
    feats = H.SequentialFeatures(past_lengths=torch.full((q.shape[0],), 61, device=dev), past_ids=past, past_embeddings=None, past_payloads={})
    default = H.eval_metrics_v2_from_tensors(state, model, feats, target_ids=target, filter_invalid_ids=True, include_eval_top_k_ids=True)
    for batch in (None, 7):
        exact = H.eval_metrics_v2_from_tensors(state, model, feats, target_ids=target, filter_invalid_ids=True, exact_ranks=True, user_max_batch_size=batch)
        assert set(exact) == set(default) - {"eval_top_k_ids"}
        for key in ("hr@1", "hr@5", "hr@10", "hr@50", "hr@100", "hr@200", "hr@500", "hr@1000"):
            assert torch.equal(exact[key], default[key]) and torch.equal(exact[key].cpu(), fx.t(f"F5/accuracy/{key}")), key
        for key in ("ndcg@1", "ndcg@5", "ndcg@10", "ndcg@50", "ndcg@100", "ndcg@200"):
            assert torch.equal(exact[key], default[key]), key
            assert torch.allclose(exact[key].float().cpu(), fx.t(f"F5/accuracy/{key}").float(), atol=1e-7), key
        # the default path's ranks, recovered from its ids as it recovers them, are the exact ones capped at MAX_K
        top = default["eval_top_k_ids"]
        k, max_k = top.size(1), 2500
        _, rank_idx = torch.max(torch.cat([top, target], dim=1) == target, dim=1)
        default_ranks = torch.where(rank_idx == k, max_k + 1, rank_idx + 1)
        exact_ranks = torch.round(1.0 / exact["mrr"]).to(torch.int64)
        assert torch.equal(1.0 / exact_ranks, exact["mrr"]) and int(exact_ranks.min()) >= 1 and int(exact_ranks.max()) <= n_items + 1
        assert torch.equal(torch.where(exact_ranks <= k, exact_ranks, max_k + 1), default_ranks)
    # a corpus beyond MAX_K + 61 items, where the default path's filter removes the seen ids (the fixture's 512 items all come back: the
    # reference's filter backfills what it cannot replace): the same comparison, the seen ids now leaving the rows' eligible sets
    n_big = 3_000
    Xb, idb = U.table(fx.cfg, n_big, 9, dev).unsqueeze(0), U.ids_of(n_big, dev).unsqueeze(0)
    big = H.EvalState(all_item_ids=set(idb.view(-1).tolist()), candidate_index=rails_amd.CandidateIndex(ids=idb, embeddings=Xb),
                      top_k_module=rails_amd.MoLBruteForceTopK(mol, Xb, idb))
    with torch.inference_mode():
        _, top = big.top_k_module(q, k=300)
    rows = torch.arange(q.shape[0], device=dev)
    past_b = top[:, 3:125:2].contiguous()                                # 61 of each row's top-125 ...
    at = torch.tensor([0, 1, 4, 9, 10, 49, 50, 99, 100, 119, 150, 250, 299, 7, 30, 75], device=dev)[: q.shape[0]]
    target_b = top[rows, at].unsqueeze(1).contiguous()                    # ... and targets before, among (seen: odd places from 3 on) and behind them
    feats_b = H.SequentialFeatures(past_lengths=torch.full((q.shape[0],), 61, device=dev), past_ids=past_b, past_embeddings=None, past_payloads={})
    default = H.eval_metrics_v2_from_tensors(big, model, feats_b, target_ids=target_b, filter_invalid_ids=True, include_eval_top_k_ids=True)
    exact = H.eval_metrics_v2_from_tensors(big, model, feats_b, target_ids=target_b, filter_invalid_ids=True, exact_ranks=True)
    for key in default:
        if key not in ("eval_top_k_ids", "mrr"):
            assert torch.equal(exact[key], default[key]), key
    exact_ranks = torch.round(1.0 / exact["mrr"]).to(torch.int64)
    _, rank_idx = torch.max(torch.cat([default["eval_top_k_ids"], target_b], dim=1) == target_b, dim=1)
    assert torch.equal(torch.where(exact_ranks <= 2500, exact_ranks, 2501), torch.where(rank_idx == 2500, 2501, rank_idx + 1))
    seen_target = (past_b == target_b).any(dim=1)
    assert bool(seen_target.any()) and bool((exact_ranks[seen_target] == n_big + 1).all()) and int(exact_ranks[~seen_target].max()) <= 300
    state.top_k_module = rails_amd.MoLAvgTopK(mol, X, ids.to(dev), avg_top_k=min(100, n_items))
    with pytest.raises(NotImplementedError, match="MoLAvgTopK.rank_of"):
        H.eval_metrics_v2_from_tensors(state, model, feats, target_ids=target, exact_ranks=True)
