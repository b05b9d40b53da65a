#!/usr/bin/env python3
"""Record the action sampler's outputs: tests/golden/sampler_pinned.npz.

The fixture was recorded on an MI355X from commit 3da062a, the last tree in which the sampler (k_sample,
k_head_sample) and the action kernels with a mode (k_act, k_head_act) were separate kernels.
tests/test_gpu_eval.py::test_sample_mode_is_the_old_sampler holds every later tree to it, bit for bit.

To re-record (only when the sampler's results are meant to change), on a GPU, with the library built:

    python tests/golden/record_sampler.py [OUT.npz]      # default: tests/golden/sampler_pinned.npz

It uses ops.sample, ops.head_sample and _lib only.  Per shape "MxK" of the test's SHAPES, built by its
_head_inputs (the exact tie, the zero mark logit, one legal move, mark disallowed, no legal move):

    MxK/h, w, b, mk            the inputs, so that the test does not depend on a random generator's stream
    MxK/hs_*                   ops.head_sample at seed 11, offset 5: a (actions), lp, jl, logits
    MxK/hsd_*                  the same with offset_dev = 3 (the logits do not depend on the draw: stored once)
    MxK/s_*                    ops.sample on those logits, seed 11, offset 5

4097x264 alone would take 4.5 MB: for it every array, inputs included, is stored as its SHA-256 (32 bytes), and
the test rebuilds the inputs with _head_inputs.
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "marl-maze_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from marlmaze import ops  # noqa: E402
from test_gpu_eval import DIGEST_ONLY, SHAPES, _head_inputs  # noqa: E402

SEED, OFFSET, OFFSET_DEV = 11, 5, 3


def digest(x):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(x).tobytes()).digest(), np.uint8)


def record(M, K):
    h, w, b, mk = _head_inputs(M, K)
    mk = mk.astype(np.uint8)
    dh, dw, db, dmk = (torch.as_tensor(x).cuda() for x in (h, w, b, mk))
    out = dict(h=h, w=w, b=b, mk=mk)
    off_dev = torch.tensor([OFFSET_DEV], dtype=torch.int64, device="cuda")
    for tag, od in (("hs", None), ("hsd", off_dev)):
        lg = torch.full((M, 6), float("nan"), device="cuda")
        a, lp, jl = ops.head_sample(dh, dw, db, dmk, SEED, OFFSET, logits=lg, offset_dev=od)
        out.update({tag + "_a": a, tag + "_lp": lp, tag + "_jl": jl})
        if od is None:
            out["hs_logits"] = logits = lg
        else:
            assert torch.equal(lg, logits)
    a, lp, jl = ops.sample(logits[:, :5], logits[:, 5], dmk, SEED, OFFSET)
    out.update(s_a=a, s_lp=lp, s_jl=jl)
    out = {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}
    assert not np.isnan(out["hs_logits"]).any()
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sampler_pinned.npz")
    fx = {}
    for M, K in SHAPES:
        for k, v in record(M, K).items():
            fx[f"{M}x{K}/{k}"] = digest(v) if (M, K) in DIGEST_ONLY else v
    np.savez_compressed(path, **fx)
    print(f"{path}: {len(fx)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
