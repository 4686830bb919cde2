"""bench.py's argument handling, input synthesis and --dump-outputs writer.  CPU only."""
import numpy as np
import pytest
import torch


def test_plain_run_drops_the_extra_legs():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full) == (5, 2, False)
    assert a.no_roofline and a.no_cpu_baseline and a.no_decode_record
    f = bench.parse(["--full"])
    assert not (f.no_roofline or f.no_cpu_baseline or f.no_decode_record)
    f = bench.parse(["--full", "--no-roofline"])
    assert f.no_roofline and not f.no_cpu_baseline and not f.no_decode_record
    with pytest.raises(SystemExit):  # the per-layer table comes from the profiled passes
        bench.parse(["--layers-out", "layers.tsv"])


def test_synth_inputs_equal_serial_draw():
    import bench
    from mlic_amd import synthetic
    jobs = [bench.Job(i, "MLICPP_L", 1, H, W, 40 + i) for i, (H, W) in enumerate([(64, 128)] * 3 + [(128, 64)] * 2)]
    groups = bench.batches(jobs)
    xs = bench.synth_inputs(groups, 3)()
    assert [tuple(x.shape) for x in xs] == [(len(js), 3, k[2], k[3]) for k, js in groups]
    for x, (_, js) in zip(xs, groups):
        assert torch.equal(x, torch.cat([synthetic.synth_image(j.H, j.W, j.seed) for j in js]))


def test_dump_outputs(tmp_path, monkeypatch):
    import bench
    jobs = [bench.Job(7 + i, "MLICPP_L", 1, 64, 64, i) for i in range(3)] + [bench.Job(20, "MLICPP_L", 1, 64, 128, 9)]
    groups = bench.batches(jobs)
    g = torch.Generator().manual_seed(0)
    last = {}
    for gi, ((_, _, H, W), js) in enumerate(groups):
        ys = [bytes(range(10 * gi + b, 10 * gi + b + 5)) for b in range(len(js))]
        zs = [bytes([200 + gi, b]) for b in range(len(js))]
        last[gi] = ({"strings": [ys, zs]}, {"x_hat": torch.rand(len(js), 3, H, W, generator=g)}, 0.0, 0.0)
    bench.dump_outputs(str(tmp_path / "full"), groups, last)
    got = {p.stem: np.load(p) for p in (tmp_path / "full").iterdir()}
    assert sorted(got) == ["streams", "x_hat", "y_strings", "z_strings"]
    assert got["streams"].dtype == np.float64 and got["streams"].tolist() == [[7, 5, 2], [8, 5, 2], [9, 5, 2], [20, 5, 2]]
    assert all(got[k].dtype == np.float32 for k in ("x_hat", "y_strings", "z_strings"))
    assert got["y_strings"].tolist() == [float(v) for gi in (0, 1) for b in range(len(groups[gi][1]))
                                         for v in range(10 * gi + b, 10 * gi + b + 5)]
    assert got["z_strings"].tolist() == [200, 0, 200, 1, 200, 2, 201, 0]
    whole = torch.cat([last[gi][1]["x_hat"].reshape(-1) for gi in range(len(groups))]).numpy()
    assert np.array_equal(got["x_hat"], whole)

    # over the cap: a fixed sample of positions, the same on every run, spanning both batches
    monkeypatch.setitem(bench.DUMP_CAPS, "x_hat", 1000)
    monkeypatch.setitem(bench.DUMP_CAPS, "y_strings", 8)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), groups, last, suffix="_rank1")
    s1 = {p.stem: np.load(p) for p in (tmp_path / "s1").iterdir()}
    s2 = {p.stem: np.load(p) for p in (tmp_path / "s2").iterdir()}
    assert sorted(s1) == ["streams_rank1", "x_hat_rank1", "y_strings_rank1", "z_strings_rank1"]
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
    idx = bench._dump_sample(whole.size, 1000, 3)
    assert s1["x_hat_rank1"].shape == (1000,) and np.array_equal(s1["x_hat_rank1"], whole[idx])
    assert idx.min() < 3 * 3 * 64 * 64 <= idx.max()
    assert s1["y_strings_rank1"].shape == (8,)
