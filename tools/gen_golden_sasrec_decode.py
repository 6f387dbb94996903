#!/usr/bin/env python3
"""Golden vectors for SASRec's cached incremental decoding: runs the REFERENCE `SASRec.encode` (modeling/sequential/sasrec.py,
imported unmodified from a reference checkout; torch only) on CPU over an append chain at each of the four SASRec fixture
geometries, and writes tests/golden/sasrec_decode_<geometry>.npz.

  python tools/gen_golden_sasrec_decode.py [--reference PATH]      (default PATH: $RAILS_REFERENCE or ../reference next to the repo)

The reference has no cache API; the contract of a decode step is "the same answer as encode of the updated sequence", so the file
records that answer.  The weights are those of tests/golden/sasrec_<geometry>.npz (loaded into the reference module, not stored
again).  The chain starts from that fixture's lengths and ids (step 0, the prefill), then appends three items: per step, every
sequence of length L < N gets a new id at position L and its length becomes L + 1; a sequence already at length N has its last id
replaced (the replace-last form of the same call).  The fixtures' row 0 is at length N (replace-last at every step) and row 1
starts at length 1 (its first step decodes position 1 against a single cached row).  At step 2 the id appended to row 2 is 0 (the
masked-row quirk: the new row's output is zero before the postprocessor, but it stays a key of every later row).
Stored: chain/lengths (S, B), chain/ids (S, B, N) int16, chain/out (S, B, D) float32 -- the reference's encode at each step.
Output files are byte-for-byte reproducible (oracle._npz.savez_deterministic).
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle._npz import savez_deterministic  # noqa: E402
from tests import _sasrec_ref as S  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
STEPS = 3          # appended items after the prefill
ZERO_ROW, ZERO_STEP = 2, 2


def append_chain(lengths, ids, num_items, seed):
    """[(lengths, ids)] for the prefill and each of the STEPS appended items."""
    g = torch.Generator().manual_seed(seed)
    N = ids.shape[1]
    chain = [(lengths.clone(), ids.clone())]
    for step in range(1, STEPS + 1):
        lengths, ids = lengths.clone(), ids.clone()
        new = torch.randint(1, num_items + 1, (ids.shape[0],), generator=g, dtype=torch.int64)
        if step == ZERO_STEP:
            new[ZERO_ROW] = 0
        for b in range(ids.shape[0]):
            if int(lengths[b]) < N:
                lengths[b] += 1
            ids[b, int(lengths[b]) - 1] = new[b]
        chain.append((lengths, ids))
    return chain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("RAILS_REFERENCE", os.path.join(os.path.dirname(REPO), "reference")))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from modeling.sequential.embedding_modules import LocalEmbeddingModule  # (reference)
    from modeling.sequential.input_features_preprocessors import LearnablePositionalEmbeddingInputFeaturesPreprocessor
    from modeling.sequential.output_postprocessors import L2NormEmbeddingPostprocessor, LayerNormEmbeddingPostprocessor
    from modeling.sequential.sasrec import SASRec
    torch.set_num_threads(1)   # reproducible CPU reductions
    for i, name in enumerate(S.GEOMETRIES):
        f = S.load(name)
        c = f["cfg"]
        D = c["D"]
        post = (LayerNormEmbeddingPostprocessor(embedding_dim=D, eps=1e-6) if c["postproc"] == "layer_norm"
                else L2NormEmbeddingPostprocessor(embedding_dim=D, eps=1e-6))
        model = SASRec(max_sequence_len=c["max_sequence_len"], max_output_len=c["max_output_len"], embedding_dim=D, num_blocks=c["blocks"],
                       num_heads=c["heads"], ffn_hidden_dim=c["ffn"], ffn_activation_fn=c["act"], ffn_dropout_rate=0.2,
                       embedding_module=LocalEmbeddingModule(num_items=c["num_items"], item_embedding_dim=D), similarity_module=None,
                       input_features_preproc_module=LearnablePositionalEmbeddingInputFeaturesPreprocessor(
                           max_sequence_len=c["N"], embedding_dim=D, dropout_rate=0.2),
                       output_postproc_module=post, activation_checkpoint=False, verbose=False)
        model.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in f.items() if k.startswith("w/")}, strict=True)
        model.eval()
        chain = append_chain(torch.from_numpy(f["in/past_lengths"]), torch.from_numpy(f["in/past_ids"]), c["num_items"], seed=31 + i)
        outs = []
        with torch.inference_mode():
            for lengths, ids in chain:
                emb = model.get_item_embeddings(ids)
                outs.append(model.encode(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads={}))
        arrays = {"chain/lengths": torch.stack([l for l, _ in chain]).numpy(),
                  "chain/ids": torch.stack([x for _, x in chain]).to(torch.int16).numpy(),
                  "chain/out": torch.stack(outs).numpy()}
        path = os.path.join(OUT, f"sasrec_decode_{name}.npz")
        savez_deterministic(path, **arrays)
        print(f"wrote tests/golden/sasrec_decode_{name}.npz ({os.path.getsize(path) // 1024} KB)")


if __name__ == "__main__":
    main()
