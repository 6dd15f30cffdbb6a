"""Generate tests/golden/flow_eval.npz by running the REFERENCE's evaluate_flow
and resize_flow (utils/flow_utils.py:62-71, 117-201).

Run where a checkout of the reference is at hand (it is imported, never copied):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval.py /path/to/reference

cv2 and imageio are not needed by the two functions: stub modules are installed
for the import of utils.flow_utils only.

What it captures per case of tests/eval_util.CASES (the reference's own code,
numpy + torch CPU fp32; data only, a few KB):

``<case>_shape`` (B, h, w), ``<case>_sizes`` [B,2], ``<case>_seed``;
``<case>_ret7``   evaluate_flow(gts, pred, moving_masks): the 7 returned numbers;
``<case>_ret5``   the same call without moving masks: 5 numbers;
``<case>_ret1``   the same case with 2-channel ground truth: 1 number;
``<case>_sample7`` [B,7] / ``<case>_sample1`` [B]: the same calls on every sample
                  alone (a batch of one), what the per-sample metrics are held to;
``<case>_bad``    [B,2] int64: the fp64 restatement's bad-pixel counts under the
                  valid and the noc mask;
``<case>_resized_<b>`` (the two small cases): resize_flow(pred[b], (H_b, W_b)).

It asserts that the reference's Fl rates equal the fp64 restatement's exactly
(the generator removed the only pixels at which fp32 rounding could flip a
count) and prints how far the reference's fp32 EPE numbers are from fp64.
The inputs are not stored: tests/eval_util regenerates them from the seeds.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import eval_util  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = Path(sys.argv[1]).resolve()
    sys.path.insert(0, str(ref))
    for name in ("cv2", "imageio"):
        sys.modules.setdefault(name, types.ModuleType(name))
    from utils.flow_utils import evaluate_flow, resize_flow

    out = {}
    worst = 0.0
    for name in eval_util.CASES:
        c = eval_util.case(name)
        pred_nhwc = np.ascontiguousarray(c["pred"].transpose(0, 2, 3, 1))
        gts, moves = c["gts"], c["moves"]
        gts2 = [np.ascontiguousarray(g[..., :2]) for g in gts]
        ret7 = evaluate_flow(gts, pred_nhwc, moves)
        ret5 = evaluate_flow(gts, pred_nhwc)
        ret1 = evaluate_flow(gts2, pred_nhwc)
        assert len(ret7) == 7 and len(ret5) == 5 and len(ret1) == 1 and ret5 == ret7[:5]
        sample7 = np.array([evaluate_flow([gts[b]], pred_nhwc[b:b + 1], [moves[b]]) for b in range(c["B"])],
                           dtype=np.float64)
        sample1 = np.array([evaluate_flow([gts2[b]], pred_nhwc[b:b + 1])[0] for b in range(c["B"])], dtype=np.float64)
        m64, bad = eval_util.evaluate_f64(c["pred"], gts, moves)
        m64_2, _ = eval_util.evaluate_f64(c["pred"], gts2)
        # the rates: exactly the fp64 restatement's
        assert np.array_equal(sample7[:, 3:5], m64[:, 3:5]), (name, sample7[:, 3:5], m64[:, 3:5])
        epe_cols = [0, 1, 2, 5, 6]
        rel = float(np.max(np.abs(sample7[:, epe_cols] - m64[:, epe_cols]) / np.abs(m64[:, epe_cols])))
        rel = max(rel, float(np.max(np.abs(sample1 - m64_2[:, 0]) / m64_2[:, 0])))
        worst = max(worst, rel)
        h, w = c["hw"]
        out[f"{name}_shape"] = np.array([c["B"], h, w], dtype=np.int64)
        out[f"{name}_sizes"] = c["sizes"].astype(np.int64)
        out[f"{name}_seed"] = np.int64(eval_util.CASES[name][3])
        out[f"{name}_ret7"] = np.array(ret7, dtype=np.float64)
        out[f"{name}_ret5"] = np.array(ret5, dtype=np.float64)
        out[f"{name}_ret1"] = np.array(ret1, dtype=np.float64)
        out[f"{name}_sample7"] = sample7
        out[f"{name}_sample1"] = sample1
        out[f"{name}_bad"] = bad
        if name in eval_util.SMALL:
            for b, (H, W) in enumerate(c["sizes"]):
                r = resize_flow(torch.from_numpy(c["pred"][b:b + 1].copy()), (int(H), int(W)))
                out[f"{name}_resized_{b}"] = r[0].numpy().astype(np.float32)
                d = float(np.max(np.abs(r[0].numpy() - eval_util.resize_f64(c["pred"][b], int(H), int(W)))))
                assert d < 1e-5, (name, b, d)
        print(f"{name}: invalidated {c['invalidated']} of {c['valid_before']} valid pixels; "
              f"reference fp32 vs fp64 EPE, max relative {rel:.2e}; bad counts {bad.tolist()}")
    path = HERE / "flow_eval.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes; worst relative deviation of the reference from fp64", f"{worst:.2e}")
    assert path.stat().st_size < 64 * 1024


if __name__ == "__main__":
    main()
