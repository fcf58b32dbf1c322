"""lbm_runner --scalar FILE --transport BWxBH: transport_state.dat holds lbm_scalar_store_binned of the
run (include/lbm_transport_hip.h), bit for bit what Engine.scalar_binned gives after the same coupled
run through the binding; the option is refused without --scalar and on --device cpu."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from conftest import GOLD, PKG
from lbm_amd import io as lio

pytestmark = pytest.mark.gpu


def test_runner_transport_option(gpu_lib, tmp_path):
    exe = PKG / "build" / "lbm_runner"
    help_text = subprocess.run([str(exe), "--help"], capture_output=True, text=True, timeout=60)
    assert "--transport" in help_text.stdout + help_text.stderr
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "23"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    p = lio.Params.from_file(str(params))
    obst = lio.read_obstacles(p.nx, p.ny, str(obst_file))
    src = [(10, 64, 2.0, 1), (40, 40, 1.0, 0), (41, 40, 0.5, 0), (127, 127, 0.25, 0)]
    (tmp_path / "dye.txt").write_text("".join(f"{x} {y} {v!r}" + (" 1\n" if f else "\n") for x, y, v, f in src))
    base = [str(exe), "--runs", "0", "--params", str(params), "--obstacles", str(obst_file)]
    scalar = ["--scalar", str(tmp_path / "dye.txt"), "--scalar-omega", "1.3"]
    bw, bh = 24, 128                                         # a ragged last bin along x; whole columns
    r = subprocess.run(base + scalar + ["--transport", f"{bw}x{bh}", "--out-dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "==done==" in r.stdout
    nbx, nby = -(-p.nx // bw), -(-p.ny // bh)
    text = (tmp_path / "transport_state.dat").read_text().splitlines()
    assert len(text) == nbx * nby and all(len(t.split()) == 3 + len(lio.SBIN_FIELDS) for t in text)
    assert text[1].split()[:2] == ["1", "0"]
    got = lio.read_transport_state(str(tmp_path / "transport_state.dat"), nbx, nby)
    phi0 = np.zeros((p.ny, p.nx), np.float32)
    for x, y, v, _ in src:
        phi0[y, x] = v
    with gpu_lib.Engine(p, obst) as e:                       # the same coupled run through the binding
        e.load_cells(lio.init_cells(p))
        e.scalar_begin(phi0, omega_s=1.3)
        e.scalar_fix(np.array([10]), np.array([64]), np.array([2.0], np.float32))
        e.run_scalar(23, 1, accelerate_first=True)
        want = e.scalar_binned(bw, bh)
    assert set(got) == set(want)
    assert np.array_equal(got["fluid"], want["fluid"])
    for name in lio.SBIN_FIELDS:
        assert np.array_equal(got[name].view(np.uint64), want[name].view(np.uint64)), name
    assert np.abs(want["fx"]).max() > 0 and want["phi"].sum() > 1
    # refused: without --scalar, on the CPU, and with bins outside the grid
    for args, word in ((["--transport", "8x8"], "--scalar"),
                       (scalar + ["--transport", "8x8", "--device", "cpu"], "--transport"),
                       (scalar + ["--transport", "0x8"], "--transport"),
                       (scalar + ["--transport", "8x129"], "--transport")):
        r = subprocess.run(base + args + ["--out-dir", str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)
