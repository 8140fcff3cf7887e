"""extract_towers on resident records while the background writer has not even created the file.

With ASYNC_WRITE, run_voxel_downsampling returns as soon as the records exist on the device, and extract_towers may
start before the writer thread has opened the output file.  Nothing on that path may ask the file system about the
file (its size decided whether the box workers are started early: [Errno 2], caught, and an empty tower list).  The
writer is held at a gate here until extract_towers has its points, so the order is the same on every run."""
import os
import threading

import numpy as np
import pytest

from pointcloudhookup_amd import las, synth

pytestmark = pytest.mark.gpu

SCALES = np.array([0.001, 0.001, 0.001])
OFFSETS = np.array([437000.0, 3139000.0, 0.0])


def test_extract_towers_on_resident_records_before_the_writer_made_the_file(cuda, tmp_path, monkeypatch):
    from pointcloudhookup_amd import las as _las
    from pointcloudhookup_amd.ui import import_PC
    from pointcloudhookup_amd.utils import tower_extraction as te
    pts = synth.corridor_numpy(400_000, seed=synth.SEED0, kind="corridor", offset=True, towers=3)
    XYZ = np.round((pts - OFFSETS) / SCALES).astype(np.int32)
    path = str(tmp_path / "cloud.las")
    las.write(path, las.LasHeader(point_format=3, version=(1, 2), scales=SCALES, offsets=OFFSETS), XYZ)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(import_PC, "ASYNC_WRITE", True)
    monkeypatch.setenv("PCH_RESIDENT_HANDOFF", "1")
    gate = threading.Event()
    real_write = _las.write_device
    monkeypatch.setattr(_las, "write_device", lambda *a, **k: (gate.wait(30), real_write(*a, **k))[1])
    out = str(tmp_path / "output" / "point_2.las")
    import_PC.run_voxel_downsampling(path, out, 0.1, 500000)
    assert not os.path.exists(out)                       # the writer waits at the gate
    logs = []

    def log(msg):
        logs.append(str(msg))
        if "总点数" in logs[-1] or "文件读取失败" in logs[-1]:   # the points are there (or the read gave up): let the writer go
            gate.set()

    got = te.extract_towers(out, log_callback=log)       # joins the writer before it returns
    assert gate.is_set() and os.path.exists(out)
    assert not any("文件读取失败" in m for m in logs), logs
    want = te.extract_towers(out, log_callback=lambda m: None)     # the entry is consumed: this one reads the file
    assert len(want) >= 1 and len(got) == len(want)
    for x, y in zip(want, got):
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k
