"""bench.py --dump-outputs on CPU tensors: dotted names for nested outputs, float32 / float64 only, a fixed seeded sample of a large array, and the
64 MB bound on everything written."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_names_dtypes_and_sample(tmp_path):
    g = torch.Generator().manual_seed(0)
    out = {"loss": torch.tensor(1.5), "kdl_terms": {"txt_emb": torch.tensor(0.25, dtype=torch.float64)},
           "outputs": {"fused_logits": torch.randn(4, 7, generator=g).to(torch.bfloat16), "labels": torch.arange(6, dtype=torch.int32),
                       "cfp": (torch.randn(3, generator=g), torch.randn(2, 2, generator=g)), "predict": None,
                       "plan": {"txt_ids": torch.arange(5)}}}
    w = torch.randn(B.DUMP_SAMPLE + 12345, generator=g)
    B.dump_outputs(str(tmp_path / "a"), out, w)
    B.dump_outputs(str(tmp_path / "b"), out, w)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["out.kdl_terms.txt_emb", "out.loss", "out.outputs.cfp.0", "out.outputs.cfp.1", "out.outputs.fused_logits",
                         "out.outputs.labels", "student_master_weights"]
    assert a["out.loss"].dtype == np.float32 and float(a["out.loss"]) == 1.5
    assert a["out.kdl_terms.txt_emb"].dtype == np.float64 and a["out.outputs.labels"].dtype == np.float64
    assert a["out.outputs.fused_logits"].dtype == np.float32 and a["out.outputs.fused_logits"].size == 28
    assert np.array_equal(a["out.outputs.labels"], np.arange(6))
    s = a["student_master_weights"]
    assert s.size == B.DUMP_SAMPLE and np.isin(s, w.numpy()).all()
    for k in a:                     # same arguments, same files
        assert np.array_equal(a[k], b[k]), k


def test_dump_stays_within_64_mb(tmp_path):
    out = {"outputs": {f"x{i}": torch.zeros(3 << 20) for i in range(20)}}
    B.dump_outputs(str(tmp_path), out, torch.zeros(10 << 20))
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 64 << 20
    assert len(os.listdir(tmp_path)) == 21
