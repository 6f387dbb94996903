#!/usr/bin/env python3
"""Golden vectors for the SASRec query encoder: runs the REFERENCE `SASRec.forward` / `SASRec.encode`
(modeling/sequential/sasrec.py, imported unmodified from a reference checkout; torch only, no shims) on CPU with seeded
parameters and inputs, and writes tests/golden/sasrec_<geometry>.npz: the inputs, every state_dict entry under `w/`, the
reference's (B, N, D) forward output and its (B, D) encode output.

  python tools/gen_golden_sasrec.py [--reference PATH]      (default PATH: $RAILS_REFERENCE or ../reference next to the repo)

Geometries (N = max_sequence_len + max_output_len = what the eval feeds):
  amzn-books     N 51,  D 64,  H 4 (hd 16), FFN 64,  4 blocks, relu, layer_norm   (sasrec-mol-*-rails-final.gin)
  amzn-books-gelu the same with gelu and l2_norm (the shipped configs all use relu; this covers the other activation)
  ml-1m          N 201, D 50,  H 1 (hd 50), FFN 50,  2 blocks, relu, l2_norm      (sasrec-sampled-softmax-*-final.gin)
  ml-20m         N 201, D 256, H 4 (hd 64), FFN 256, 1 block,  relu, layer_norm   (the shipped config has 4 blocks; one keeps the
                                                                                  fixture small and runs every kernel at this
                                                                                  geometry; chained blocks are covered by the
                                                                                  2- and 4-block fixtures above)
Every bias is re-drawn at O(0.1 - 1): the reference's init leaves the attention biases at zero, which would hide a dropped or
shifted bias.  Every other parameter (weights, item and position tables) keeps the reference's init rounded to a power-of-two grid
step of about 1/4 of the tensor's standard deviation; the reference computes on exactly these values, and the file stores them as
int8 codes under `w/<name>` with the step under `wstep/<name>` (value = code * step, exact in float32; tests/_sasrec_ref.py
decodes them), so the ml-20m fixture stays small.  For N > 64 the (B, N, D) forward output is stored at a sample of positions
(`out/sequence_positions`: every 16th, the last, each row's last valid position, the id-0 position and the nonzero ids past a
length).  Inputs per fixture: lengths of 1, N and in between; one row with an id 0 inside its length; one row with nonzero ids past
its length; a small item vocabulary.  Output files are byte-for-byte reproducible (oracle._npz.savez_deterministic).
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle._npz import savez_deterministic  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")

# name: (max_sequence_len, max_output_len, D, blocks, heads, ffn, act, postproc, num_items, batch)
GEOMETRIES = {
    "amzn-books": (50, 1, 64, 4, 4, 64, "relu", "layer_norm", 200, 8),
    "amzn-books-gelu": (50, 1, 64, 4, 4, 64, "gelu", "l2_norm", 200, 8),
    "ml-1m": (200, 1, 50, 2, 1, 50, "relu", "l2_norm", 300, 8),
    "ml-20m": (200, 1, 256, 1, 4, 256, "relu", "layer_norm", 150, 4),
}


def build_reference(R, name, seed):
    msl, mol, D, blocks, heads, ffn, act, post, num_items, _ = GEOMETRIES[name]
    torch.manual_seed(seed)
    postproc = (R.LayerNormEmbeddingPostprocessor(embedding_dim=D, eps=1e-6) if post == "layer_norm"
                else R.L2NormEmbeddingPostprocessor(embedding_dim=D, eps=1e-6))
    model = R.SASRec(
        max_sequence_len=msl, max_output_len=mol, embedding_dim=D, num_blocks=blocks, num_heads=heads, ffn_hidden_dim=ffn,
        ffn_activation_fn=act, ffn_dropout_rate=0.2,
        embedding_module=R.LocalEmbeddingModule(num_items=num_items, item_embedding_dim=D),
        similarity_module=None,
        input_features_preproc_module=R.LearnablePositionalEmbeddingInputFeaturesPreprocessor(max_sequence_len=msl + mol, embedding_dim=D,
                                                                                               dropout_rate=0.2),
        output_postproc_module=postproc, activation_checkpoint=False, verbose=False)
    model.eval()
    g = torch.Generator().manual_seed(seed + 1)
    steps = {}
    with torch.no_grad():
        for pname, p in sorted(model.named_parameters()):
            if pname.endswith("bias"):
                p.copy_((torch.rand(p.shape, generator=g) * 0.9 + 0.1) * torch.where(torch.rand(p.shape, generator=g) < 0.5, -1.0, 1.0))
            else:
                steps[pname] = step = 2.0 ** float(torch.floor(torch.log2(p.std() / 4)))
                p.copy_(torch.round(p / step) * step)
    return model, steps


def sequence_positions(lengths, ids):
    N = ids.shape[1]
    if N <= 64:
        return torch.arange(N)
    pos = set(range(0, N, 16)) | {N - 1}
    for b in range(ids.shape[0]):
        n = int(lengths[b])
        pos.add(n - 1)
        pos |= {int(j) for j in (ids[b, :n] == 0).nonzero()[:, 0]}          # id 0 inside the length
        pos |= {n + int(j) for j in (ids[b, n:] != 0).nonzero()[:, 0]}      # nonzero ids past the length
    return torch.tensor(sorted(pos), dtype=torch.int64)


def make_inputs(name, seed):
    msl, mol, _, _, _, _, _, _, num_items, B = GEOMETRIES[name]
    N = msl + mol
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(2, N, (B,), generator=g, dtype=torch.int64)
    lengths[0] = N          # a full row
    lengths[1] = 1          # the shortest possible
    ids = torch.randint(1, num_items + 1, (B, N), generator=g, dtype=torch.int64)
    ids = ids * (torch.arange(N).unsqueeze(0) < lengths.unsqueeze(1))
    ids[2, int(lengths[2]) // 2] = 0                                   # an id 0 inside the length: a masked row that is still a key
    tail = int(lengths[3])
    ids[3, tail:min(N, tail + 5)] = torch.randint(1, num_items + 1, (min(N, tail + 5) - tail,), generator=g)   # nonzero ids past the length
    return lengths, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("RAILS_REFERENCE", os.path.join(os.path.dirname(REPO), "reference")))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import types

    from modeling.sequential.embedding_modules import LocalEmbeddingModule  # (reference)
    from modeling.sequential.input_features_preprocessors import LearnablePositionalEmbeddingInputFeaturesPreprocessor
    from modeling.sequential.output_postprocessors import L2NormEmbeddingPostprocessor, LayerNormEmbeddingPostprocessor
    from modeling.sequential.sasrec import SASRec
    R = types.SimpleNamespace(LocalEmbeddingModule=LocalEmbeddingModule, SASRec=SASRec, L2NormEmbeddingPostprocessor=L2NormEmbeddingPostprocessor,
                              LayerNormEmbeddingPostprocessor=LayerNormEmbeddingPostprocessor,
                              LearnablePositionalEmbeddingInputFeaturesPreprocessor=LearnablePositionalEmbeddingInputFeaturesPreprocessor)
    torch.set_num_threads(1)   # reproducible CPU reductions
    os.makedirs(OUT, exist_ok=True)
    for i, name in enumerate(GEOMETRIES):
        msl, mol, D, blocks, heads, ffn, act, post, num_items, B = GEOMETRIES[name]
        model, steps = build_reference(R, name, seed=21 + i)
        lengths, ids = make_inputs(name, seed=7 + i)
        with torch.inference_mode():
            emb = model.get_item_embeddings(ids)
            seq = model.forward(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads={})
            cur = model.encode(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads={})
        pos = sequence_positions(lengths, ids)
        arrays = {"in/past_lengths": lengths.numpy(), "in/past_ids": ids.numpy(), "out/sequence_positions": pos.numpy(),
                  "out/sequence_embeddings": seq[:, pos].contiguous().numpy(), "out/current_embeddings": cur.numpy(),
                  "meta/geometry": np.array([msl, mol, D, blocks, heads, ffn, num_items], dtype=np.int64),
                  "meta/ffn_activation_fn": np.array(act), "meta/output_postproc": np.array(post)}
        for k, v in model.state_dict().items():
            if k in steps:
                step = steps[k]
                codes = torch.round(v / step)
                assert float(codes.abs().max()) <= 127 and torch.equal(codes * step, v), k
                arrays["w/" + k], arrays["wstep/" + k] = codes.to(torch.int8).numpy(), np.array(step)
            else:
                arrays["w/" + k] = v.detach().numpy()
        path = os.path.join(OUT, f"sasrec_{name}.npz")
        savez_deterministic(path, **arrays)
        print(f"wrote tests/golden/sasrec_{name}.npz ({os.path.getsize(path) // 1024} KB)")


if __name__ == "__main__":
    main()
