"""Pins oracle/swin_oracle.py against the installed `transformers` package (the reference's own dependency,
Allen_data_Backbone/train.py:70-85) and writes tests/golden/swin_<name>.npz (SWIN_CASES) and
tests/golden/swin_geom_<name>.npz (SWIN_GEOMETRIES). Build container only:

    PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden_swin.py [name ...]

Without names every case of both tables is written; with names only those (a name of SWIN_CASES first, then of
SWIN_GEOMETRIES), so fixtures that are not named are left as they are.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

import transformers  # noqa: E402
from transformers import SwinConfig, SwinForImageClassification  # noqa: E402

from oracle import swin_oracle as SO  # noqa: E402
from tests.golden_cases import SWIN_CASES, SWIN_GEOMETRIES  # noqa: E402
from vit_ocm_wmsegmentation_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def main(names):
    torch.set_num_threads(8)
    todo = [(f"swin_{n}", c) for n, c in SWIN_CASES.items()] + [(f"swin_geom_{n}", c) for n, c in SWIN_GEOMETRIES.items()]
    if names:
        unknown = [n for n in names if n not in SWIN_CASES and n not in SWIN_GEOMETRIES]
        if unknown:
            raise SystemExit(f"unknown Swin case(s) {unknown}: SWIN_CASES {sorted(SWIN_CASES)}, SWIN_GEOMETRIES "
                             f"{sorted(SWIN_GEOMETRIES)}")
        todo = [(f"swin_{n}", SWIN_CASES[n]) if n in SWIN_CASES else (f"swin_geom_{n}", SWIN_GEOMETRIES[n]) for n in names]
    for name, c in todo:
        cfg = dict(synth.SWIN_TINY, **c.get("cfg", {}))
        hf_cfg = SwinConfig(image_size=cfg["image_size"], patch_size=cfg["patch_size"], num_channels=cfg["num_channels"],
                            embed_dim=cfg["embed_dim"], depths=list(cfg["depths"]), num_heads=list(cfg["num_heads"]),
                            window_size=cfg["window_size"], mlp_ratio=cfg["mlp_ratio"],
                            layer_norm_eps=cfg["layer_norm_eps"], num_labels=cfg["num_labels"])
        model = SwinForImageClassification(hf_cfg).eval()
        sd = synth.synth_swin_state_dict(cfg, seed=c["seed"], qk_gain=c["qk_gain"])
        msg = model.load_state_dict(sd, strict=True)
        assert not msg.missing_keys and not msg.unexpected_keys
        x = synth.synth_tiles(c["batch"], cfg["image_size"], seed=c["seed"] + 50, channels=cfg["num_channels"])
        with torch.no_grad():
            ref = model(pixel_values=x, output_hidden_states=True)
            inner = model.swin(pixel_values=x)
        o = SO.swin_forward(sd, cfg, x)
        d = [float((ref.logits - o["logits"]).abs().max()), float((inner.pooler_output - o["pooled"]).abs().max()),
             float((inner.last_hidden_state - o["last_hidden_state"]).abs().max())]
        assert max(d) <= 2e-5, f"{name}: oracle vs transformers {d}"
        out = {"logits": ref.logits.numpy(), "pooled": inner.pooler_output.numpy(),
               "last_hidden_head": inner.last_hidden_state[:, :8, :64].numpy(),
               "last_hidden_abssum": np.float64(inner.last_hidden_state.double().abs().sum()),
               "oracle_vs_transformers_maxabs": np.float64(max(d)),
               "transformers_version": np.array(transformers.__version__)}
        for s, t in enumerate(o["stage_out"]):
            out[f"stage{s}_head"] = t[:, :4, :32].numpy()
            out[f"stage{s}_abssum"] = np.float64(t.double().abs().sum())
        path = os.path.join(GOLD, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{name:16s} oracle-vs-transformers {max(d):.2e}  logits[0, :5] {ref.logits[0, :5].numpy().round(4)} -> "
              f"{os.path.relpath(path, ROOT)} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main(sys.argv[1:])
