#!/usr/bin/env python
"""Writes tests/golden/clip_text_bitexact.pt: ClipTextEngine's output bits for one tiny configuration, as the installed library and
storygen_amd/encoders.py produce them on an MI355X.  tests/test_clip_score_gpu.py compares the engine against these bits, so a change
of the engine's launch sequence that is meant to be neutral (the layer loop shared with ClipVisionEngine) has to reproduce them.  The
committed file was written by this script on the commit BEFORE that loop was factored out.

    python tools/make_clip_text_bitexact.py [out.pt]

Two layers of 64 channels, 2 heads of 32, 77 and 24 tokens, with and without a padding mask; the weights are stored in the file, so
the test depends on no random number generator."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from storygen_amd.encoders import ClipTextEngine, clip_text_param_shapes, init_state  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "clip_text_bitexact.pt")
    sd = init_state(clip_text_param_shapes(vocab_size=96, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                                           max_position_embeddings=77), seed=23)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 95, (2, 77), generator=g)
    ids[0, 40], ids[1, 12] = 95, 95                         # the pooled row is the argmax token's
    mask = torch.ones(1, 24)
    mask[:, 19:] = 0
    eng = ClipTextEngine(sd, "cuda:0", heads=2)
    hidden, pooled = eng(ids)
    hidden_m, pooled_m = eng(ids[:1, :24], attention_mask=mask)
    torch.cuda.synchronize()
    torch.save(dict(state_dict=sd, heads=2, input_ids=ids, mask=mask, hidden=hidden.cpu(), pooled=pooled.cpu(), hidden_masked=hidden_m.cpu(),
                    pooled_masked=pooled_m.cpu()), out)
    print(f"wrote {out}: hidden {tuple(hidden.shape)} |x| max {float(hidden.abs().max()):.3f}")


if __name__ == "__main__":
    main()
