"""Generate tests/golden/scannet_ref.npz: inputs, the random numbers numpy handed out, and the outputs of the REFERENCE's own ScanNet
augmentation — `augment_fn` of scannet_seg/train_scannet.py:95-129 and the `augment_fn1` -> `augment_fn2` chain of
scannet_seg/evaluate_scannet_withoverlap.py:94-116,282-286 — on a [6, 16, 6] float32 batch, so that
``sph3d_gcn_amd/harness/scannet.py``'s float64 statement of the recipes and of the chained views can be pinned against them
(tests/test_scannet.py).

Runs in the build container only (it reads /root/reference at run time; nothing of it is copied here): utils/data_util.py is pure
numpy and is imported as it is; the two scripts import TensorFlow at the top, so the three FunctionDef nodes are taken out of their
files' ASTs, compiled and executed with ``np`` and ``data_util`` in scope — the reference's own statements, run here, not restated
(tests/golden/make_blockio_golden.py does the same).  While a function runs, np.random.uniform, randn and shuffle are wrapped so
that what they hand out is recorded; the fixture holds data only.

    python tests/golden/make_scannet_golden.py          # writes tests/golden/scannet_ref.npz

Layout of the recorded numbers, in the order the functions ask for them (bsize 6, third = 2, 16 points):
  train_shuffle    [6 + 16]   the batch permutation, then the point permutation (np.random.shuffle of an arange)
  train_random     clouds 0:2 — 2 turn uniforms, 2 x 3 tilt normals, 2 scales, 2 x 3 shifts, 2 x 16 x 3 jitter normals —, then
                   clouds 2:4 — 2 x 3 tilt normals, 2 scales, 2 x 3 shifts, 2 x 16 x 3 jitter normals
  eval1_random     6 x 3 tilt normals, 6 scales, 6 x 3 shifts, 6 x 16 x 3 jitter normals
  eval2_random     6 turn uniforms, then as eval1_random
"""
import ast
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


class Recorder:
    """np.random.uniform / randn / shuffle, recording every value they hand out"""

    def __init__(self):
        self.handed, self.shuffled = [], []
        self._uniform, self._randn, self._shuffle = np.random.uniform, np.random.randn, np.random.shuffle

    def __enter__(self):
        def uniform(*a, **k):
            v = self._uniform(*a, **k)
            self.handed.append(np.asarray(v, dtype=np.float64).reshape(-1))
            return v

        def randn(*a):
            v = self._randn(*a)
            self.handed.append(np.asarray(v, dtype=np.float64).reshape(-1))
            return v

        def shuffle(x):
            self._shuffle(x)
            self.shuffled.append(np.asarray(x, dtype=np.int64).copy())
        np.random.uniform, np.random.randn, np.random.shuffle = uniform, randn, shuffle
        return self

    def __exit__(self, *exc):
        np.random.uniform, np.random.randn, np.random.shuffle = self._uniform, self._randn, self._shuffle
        return False


def load_reference():
    sys.path.insert(0, os.path.join(REF, "utils"))
    import data_util                                           # the reference's module, unmodified
    ns = {"np": np, "data_util": data_util}
    for script, names in (("train_scannet.py", ("augment_fn",)), ("evaluate_scannet_withoverlap.py", ("augment_fn1", "augment_fn2"))):
        src = open(os.path.join(REF, "scannet_seg", script)).read()
        body = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert len(body) == len(names), (script, names)
        exec(compile(ast.Module(body=body, type_ignores=[]), script, "exec"), ns)
    return ns["augment_fn"], ns["augment_fn1"], ns["augment_fn2"]


def main():
    augment_fn, augment_fn1, augment_fn2 = load_reference()
    rng = np.random.RandomState(2026)
    bsize, n = 6, 16
    binp = np.concatenate(((rng.rand(bsize, n, 3) * 2.0 - 0.5), rng.rand(bsize, n, 3)), axis=2).astype(np.float32)
    blab = rng.randint(0, 21, (bsize, n)).astype(np.int32)
    binn = rng.randint(0, 2, (bsize, n)).astype(np.int32)
    out = {"input": binp.copy(), "label": blab.copy(), "inner": binn.copy()}
    # --- the training recipe ---
    np.random.seed(51)
    with Recorder() as rec:
        a, b, c = augment_fn(binp.copy(), blab.copy(), binn.copy())
    out["train_seed"] = np.int64(51)
    out["train_out_input"], out["train_out_label"], out["train_out_inner"] = np.asarray(a), np.asarray(b), np.asarray(c)
    out["train_shuffle"], out["train_random"] = np.concatenate(rec.shuffled), np.concatenate(rec.handed)
    # --- the evaluation's chain: fn1 on the plain batch, then fn2 on what fn1 left (the script augments in place) ---
    batch = binp.copy()
    np.random.seed(52)
    with Recorder() as rec:
        batch = augment_fn1(batch)
    out["eval_seed"] = np.int64(52)
    out["eval1_out"], out["eval1_random"] = np.asarray(batch).copy(), np.concatenate(rec.handed)
    with Recorder() as rec:
        batch = augment_fn2(batch)
    out["eval2_out"], out["eval2_random"] = np.asarray(batch).copy(), np.concatenate(rec.handed)
    path = os.path.join(HERE, "scannet_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: (v.shape, str(v.dtype)) for k, v in out.items() if hasattr(v, "shape")})


if __name__ == "__main__":
    main()
