"""bench.py --dump-outputs on the GPU: a plain run of every kind of config,
cut to N frames, writes what its last timed step computed — checked against
the oracle over the same frames (generated on the host: the same bytes) and
for being the same files in a second run; and a plain run returns the lean
line, nothing measured in runs of their own."""
import numpy as np
import pytest

import bench
import oracle
from ingot_amd import Chain, EditOp, Field, GenProfile
from ingot_amd.hostgen import gen_frames_host

N = 3001  # odd, several workgroups, a partial last one
STEPS, WARMUP = 3, 1


@pytest.fixture(scope="module")
def env():
    import torch
    import torch.distributed as dist

    import ingot_amd

    ctx = ingot_amd.Context(0)
    yield (torch, dist, ingot_amd, ingot_amd.load_library(), ctx, 1, 0, 0,
           torch.device("cuda:0"))
    comm = getattr(ctx, "_flow_comm", None)  # config 5's one-rank communicator
    if comm is not None:
        comm.close()


def _bytes(path, row_bytes):
    a = np.load(path)
    assert a.dtype == np.float64 and a.shape[1] == row_bytes // 4
    return a.astype("<u4").view(np.uint8).reshape(-1, row_bytes)


def _run(env, monkeypatch, tmp_path, config, extra=()):
    """Two plain runs of `config` over N frames -> (host frames, the first
    run's dump directory); the second run's files equal the first's."""
    prof, _, stride, chain, desc = bench.CONFIGS[config]
    monkeypatch.setitem(bench.CONFIGS, config, (prof, N, stride, chain, desc))
    for d in ("a", "b"):
        args = bench.parse_args(["--config", config, "--steps", str(STEPS), "--warmup",
                                 str(WARMUP), "--rotate-mib", "1", "--dump-outputs",
                                 str(tmp_path / d), *extra])
        line = bench.run_config(args, config, env)
        assert line["steps"] == STEPS and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["config"]["frames_per_gpu"] == N
        assert not {"roofline", "variants", "cpu_baseline", "host_inclusive",
                    "ms_per_step_ungated"} & set(line)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "b").iterdir()) and names
    for name in names:
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
    assert not any(name.endswith("_rows.npy") for name in names)  # N frames fit the budget
    return gen_frames_host(GenProfile[prof], N, stride=stride), tmp_path / "a"


@pytest.mark.gpu
@pytest.mark.parametrize("config,extra", [("c2", ()), ("c2", ("--timing", "ring")),
                                          ("c3p", ()), ("c3r", ()), ("c2r", ())],
                         ids=["c2", "c2-ring", "c3p", "c3r", "c2r"])
def test_dumped_records_are_the_oracles(env, monkeypatch, tmp_path, config, extra):
    """Per-batch launches, the ring consumer, lengths-only packed frames and
    parse_read over chunk lists (no header straddles a cut): the records of
    step K - 1 are parse_slice's over the batch."""
    (arena, off, lens), d = _run(env, monkeypatch, tmp_path, config, extra)
    _, _, stride, chain, _ = bench.CONFIGS[config]
    want = oracle.parse_batch(arena, off, lens, Chain[chain], stride=stride or 0, n=N)
    got = _bytes(d / "records.npy", 16)
    assert got.shape == (N, 16)
    assert (got == want.view(np.uint8).reshape(N, 16)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [(), ("--timing", "ring")], ids=["launches", "ring"])
def test_dumped_compact_records_are_a_direct_parse(env, monkeypatch, tmp_path, extra):
    """--record 8: the dump is the n x 8 B the step wrote, equal to
    parse_strided_compact over the same frames."""
    _run(env, monkeypatch, tmp_path, "c2", ("--record", "8", *extra))
    torch, ingot_amd, ctx = env[0], env[2], env[4]
    arena, _, _ = ingot_amd.gen_frames(GenProfile.V4UDP64, N, stride=64)
    want = ctx.parse_strided_compact(arena, 64, N, Chain.UdpParser)
    torch.cuda.synchronize()
    got = _bytes(tmp_path / "a" / "records.npy", 8)
    assert got.shape == (N, 8)
    assert (got == want.cpu().numpy().view(np.uint8).reshape(N, 8)).all()


@pytest.mark.gpu
def test_dumped_frames_after_modify(env, monkeypatch, tmp_path):
    """c2m: step K - 1 rewrote arena copy (K - 1) % R in place, which no
    earlier step of this run touched (W + K <= R): the frames with the UDP
    destination decremented once."""
    (arena, _, _), d = _run(env, monkeypatch, tmp_path, "c2m")
    want = arena.copy()
    oracle.parse_modify_batch(want, None, None, Chain.UdpParser,
                              [(2, Field.UDP_DESTINATION, EditOp.SUB, 1)], stride=64, n=N)
    assert (want[:N * 64] != arena[:N * 64]).any()
    got = _bytes(d / "frames.npy", 64)
    assert got.shape == (N, 64)
    assert (got == want[:N * 64].reshape(N, 64)).all()


@pytest.mark.gpu
def test_dumped_flow_histogram_and_ids(env, monkeypatch, tmp_path):
    """c5: the reduced histogram (one rank) and the per-packet flow bins."""
    (arena, off, lens), d = _run(env, monkeypatch, tmp_path, "c5")
    want = np.zeros(bench.FLOW_BINS, np.uint32)
    oracle.flow_hist(arena, off, lens, Chain.VlanUlp, bins=bench.FLOW_BINS, hist=want)
    hist = np.load(d / "flow_hist.npy")
    assert hist.shape == (bench.FLOW_BINS, 1) and (hist[:, 0] == want).all() and want.sum() > 0
    ids = np.load(d / "flow_ids.npy")
    assert ids.shape == (N, 1) and (ids[:, 0] == oracle.flow_hist.last_flows).all()


@pytest.mark.gpu
def test_dumped_emitted_packets(env, monkeypatch, tmp_path):
    """c6e: the packed destination arena in 64-B rows (the bytes past the
    last whole row are left out), equal to the oracle's Emit."""
    (arena, off, lens), d = _run(env, monkeypatch, tmp_path, "c6e")
    hdr, sets = bench.emit_stack()
    ports, vnis = bench.emit_values(N)
    ln = lens.astype(np.int64) + len(hdr)
    d_off = np.cumsum(ln) - ln
    want = np.zeros(int(ln.sum()) + 64, np.uint8)
    oracle.emit_batch(hdr, [sets[0], sets[1], (*sets[2], ports), (*sets[3], vnis)], arena, off,
                      lens, want, d_off)
    rows = int(ln.sum()) // 64
    got = _bytes(d / "emitted.npy", 64)
    assert got.shape == (rows, 64)
    assert (got == want[:rows * 64].reshape(rows, 64)).all()
