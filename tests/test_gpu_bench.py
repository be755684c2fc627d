"""bench.py on a small genome: a plain run times exactly --steps steps, measures nothing besides the headline, and
--dump-outputs writes the last timed step's compact answer in float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--genome-size", "2e6", "--queries", "2000", "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(dump), "--detail-out", str(tmp_path / "detail.json")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.rstrip("\n").splitlines()[-1])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"] == "u32" and out["higher_is_better"] is True
    detail = json.load(open(tmp_path / "detail.json"))
    for k in ("sustained", "value_same_batch", "value_one_in_flight", "value_with_d2h", "cli_end_to_end", "extra_configs"):
        assert k not in detail, k
    assert detail["cpu_baseline"] is None and detail["parity_sample"] is None
    got = {k: np.load(dump / (k + ".npy")) for k in ("hit_counts", "query_info", "hit_query", "hit_records")}
    assert all(v.dtype == np.float64 for v in got.values())
    counts = got["hit_counts"]
    assert len(counts) == len(got["query_info"]) == 2000 and counts.sum() > 0
    assert len(got["hit_query"]) == len(got["hit_records"]) == counts.sum() == detail["hits_per_step"]
    assert np.array_equal(np.bincount(got["hit_query"].astype(np.int64), minlength=2000), counts)
