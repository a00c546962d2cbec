"""bench.py's plain run and --dump-outputs on a small job (2 channels): the
line carries the headline and ms_per_step for exactly --steps timed steps and
none of the --full legs, and the dumped rows are the float32 magnitude rows of
the seeded input at the rows dump_row_ids names (checked against NumPy f64 with
the tolerance of the benchmark's own row check, first and zero-padded last
frames included)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = 2


@pytest.fixture(scope="module")
def bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench as b
    return b


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--channels", str(CH),
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), d


def test_plain_line_is_lean(plain_run):
    line, _ = plain_run
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    # value = frames of the timed steps / their wall time, ms_per_step = that wall time / steps
    fps = line["config"]["frames_per_step"] / (line["ms_per_step"] * 1e-3)
    assert abs(fps - line["value"]) <= 1e-3 * line["value"]
    for leg in ("cpu_baseline", "config5_shard_32ch", "fft_c2c_1024", "fir_ols_257", "stft_config3",
                "stft_sizes", "features"):
        assert leg not in line
    assert line["check_row_vs_numpy_f64"] is None


def test_dumped_rows_match_f64(plain_run, bench):
    import torch
    _, d = plain_run
    files = sorted(os.listdir(d))
    assert files == [bench.DUMP_NAME + ".npy"]
    rows = np.load(os.path.join(d, files[0]))
    nfr = bench.frames_of(bench.SAMPLES)
    ids = bench.dump_row_ids(CH, nfr)
    assert rows.dtype == np.float32 and rows.shape == (len(ids), bench.NFFT)
    assert rows.nbytes <= 64 * 1024 * 1024 and len(ids) == bench.DUMP_ROWS
    assert np.array_equal(ids, bench.dump_row_ids(CH, nfr)) and np.all(np.diff(ids) > 0)
    for edge in (0, nfr - 1, (CH - 1) * nfr, CH * nfr - 1):
        assert edge in ids
    w = bench.hann64()
    for c in range(CH):
        sig = torch.empty(bench.SAMPLES, device="cuda")
        sig.uniform_(-1.0, 1.0, generator=torch.Generator(device="cuda").manual_seed(c))
        x = np.concatenate([sig.cpu().numpy().astype(np.float64), np.zeros(bench.NFFT)])
        del sig
        mine = np.nonzero(ids // nfr == c)[0]
        for k in np.concatenate([mine[:2], mine[len(mine) // 2:len(mine) // 2 + 2], mine[-2:]]):
            fr = int(ids[k] % nfr)
            want = np.abs(np.fft.fft(x[fr * bench.HOP: fr * bench.HOP + bench.NFFT] * w))
            np.testing.assert_allclose(rows[k], want, rtol=5e-5, atol=5e-5)
