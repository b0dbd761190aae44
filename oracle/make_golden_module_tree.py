#!/usr/bin/env python
"""TEST INFRASTRUCTURE — records the module tree of the reference's own UNet2DConditionModel (model/unet_2d_condition.py, imported
verbatim on oracle/diffusers_shim) at the small config of tests/test_dropin.py and writes tests/golden/tiny_module_tree.json:
state-dict keys in order with their shapes, the attn3 module names and their parameter count.

    python oracle/make_golden_module_tree.py        # needs the reference tree (STORYGEN_REFERENCE); build container only

tests/test_dropin.py::test_state_dict_matches_the_reference_module_tree checks storygen_amd.model against the file."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_runner import import_reference  # noqa: E402

TINY = dict(block_out_channels=(32, 64), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
            up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), cross_attention_dim=48, sample_size=64)


def main():
    RefUNet, _, _ = import_reference()
    ref = RefUNet(**TINY)
    attn3 = sorted(n for n, _ in ref.named_modules() if n.endswith("attn3"))
    out = {"config": TINY, "made_by": "oracle/make_golden_module_tree.py",
           "state_dict": [[k, list(v.shape)] for k, v in ref.state_dict().items()],
           "attn3_modules": attn3,
           "attn3_parameters": sum(p.numel() for n, m in ref.named_modules() if n.endswith("attn3") for p in m.parameters())}
    path = os.path.join(ROOT, "tests", "golden", "tiny_module_tree.json")
    rows = ",\n".join(f"  [{json.dumps(k)}, {json.dumps(shape)}]" for k, shape in out["state_dict"])     # one key per line
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: " + (f"[\n{rows}\n ]" if k == "state_dict" else json.dumps(v))
                                   for k, v in out.items()) + "\n}\n")
    print(f"wrote {path}: {len(out['state_dict'])} keys, {len(attn3)} attn3 modules")


if __name__ == "__main__":
    main()
