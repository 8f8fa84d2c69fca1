"""GPU: every reader (and the one writer) of the lattice parameters is held to the all-gather the step before left in flight.

`Trainer.step` returns with the all-gather of the three lattices' updated parameters still running (sharded optimiser,
`defer_param_gather`); the rule at `Trainer._params_ready` is that whatever READS a lattice waits for its gather first, and that
no gather outlives the next optimiser step, which WRITES the tables.  tests/test_gpu_dp_schedule.py runs the schedule under the
timed `parallel.Loopback`: the table holds NaN for `delay_cycles` and is restored whether or not anybody waited, so a reader
that forgot to wait is caught only if it happens to run inside that window -- and values that are dropped again (the SDFs the
importance sampler places its samples from) never reach the loss at all.  Here the double runs with `hold=True`: the table (and,
for the lattices' early reductions, the gradient buffer) holds NaN from the launch until `wait()`, whatever the timing.  A NaN
read is arithmetic; nothing here provokes a fault.

Every test uses the small step of test_gpu_train_step.py::test_step_without_foreground_samples (128 rays, a 2-image 40 x 60
reel), Loopback(world=2, delay_cycles=100_000, hold=True) and a deferred gather."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

LATTICES = ("sdf", "rgb", "bg")       # lattice index 0, 1, 2 of Trainer._pending_gather


@contextlib.contextmanager
def _loopback(hold=True, serialize=False):
    """the double of every test here, installed; the previous one comes back whatever happens"""
    from permuto_sdf_amd import parallel
    lb = parallel.Loopback(world=2, delay_cycles=100_000, serialize=serialize, hold=hold)
    prev = parallel.set_loopback(lb)
    try:
        yield lb
    finally:
        parallel.set_loopback(prev)


def _reset_jitter_streams():
    from permuto_sdf_amd import bridge
    for cls in (bridge.OccupancyGrid, bridge.RaySampler, bridge.VolumeRendering):     # the process-global jitter streams
        cls._rng = bridge.Pcg32()


def _hp():
    from permuto_sdf_amd.train_step import HyperParams
    hp = HyperParams()
    hp.nr_rays, hp.target_nr_of_samples = 128, 128 * 96
    return hp


def _reel(dev):
    from permuto_sdf_amd.train_step import SyntheticReel
    return SyntheticReel(dev, nr_images=2, height=40, width=60)


def _trainer(dev, kind="manual", start_iter=1, defer=True):
    from permuto_sdf_amd.train_manual import ManualTrainer
    from permuto_sdf_amd.train_step import Trainer
    _reset_jitter_streams()
    torch.manual_seed(0)
    if kind == "autograd":
        tr = Trainer(dev, _hp())
    else:
        tr = ManualTrainer(dev, _hp(), with_mask=(kind == "masked"))
    tr.defer_param_gather = defer
    tr.iter = start_iter
    return tr


def _tables(tr):
    return [getattr(tr, name).encoding.lattice_values for name in LATTICES]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ================================================================================================== the double itself
def test_hold_keeps_nan_in_the_table_until_wait_on_whatever_stream_waits(dev):
    from permuto_sdf_amd import parallel
    g = torch.Generator().manual_seed(5)
    table = torch.randn(4096, generator=g).to(dev)
    orig = table.clone()
    torch.cuda.synchronize()
    with _loopback() as lb:
        su = parallel.ShardedUpdate()
        su.all_gather(table, (0, 2048))
        torch.cuda.synchronize()                   # far past delay_cycles: nobody waited, so nothing came back
        assert bool(torch.isnan(table).all())
        su.wait()
        torch.cuda.synchronize()
        assert torch.equal(_bits(table), _bits(orig))
        # wait() on a non-default stream: the table is restored ON that stream, a read on it sees the original
        su.all_gather(table, (0, 2048))
        torch.cuda.synchronize()
        assert bool(torch.isnan(table).all())
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            su.wait()
            seen = table.clone()
        side.synchronize()
        assert torch.equal(_bits(seen), _bits(orig))
        torch.cuda.synchronize()
        assert torch.equal(_bits(table), _bits(orig))
        assert [k for k, _ in lb.launched] == ["all_gather_params"] * 2


def test_hold_reduces_what_the_buffer_held_at_launch(dev):
    """the lattices' early reductions (ShardedUpdate.reduce_scatter -> Loopback.all_reduce): an add issued after the launch is
    lost every time, a consumer that did not wait reads NaN"""
    from permuto_sdf_amd import parallel
    g = torch.Generator().manual_seed(6)
    buf = torch.randn(4096, generator=g).to(dev)
    at_launch = buf.clone()
    torch.cuda.synchronize()
    with _loopback() as lb:
        su = parallel.ShardedUpdate()
        assert su.reduce_scatter(buf) == (0, 2048)
        buf.add_(1.0)                              # a kernel that still adds to the gradient after its reduction was started
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all())
        su.wait()
        torch.cuda.synchronize()
        assert torch.equal(_bits(buf), _bits(at_launch * lb.world))
        # serialize=True keeps its meaning under hold: waited for at once, so the sum is there at once
    with _loopback(serialize=True) as lb:
        buf.copy_(at_launch)
        w = lb.all_reduce(buf)
        torch.cuda.synchronize()
        assert torch.equal(_bits(buf), _bits(at_launch * lb.world))
        table = at_launch.clone()
        lb.gather_params(table)
        torch.cuda.synchronize()
        assert torch.equal(_bits(table), _bits(at_launch))
        w.wait()                                   # a second wait changes nothing
        torch.cuda.synchronize()
        assert torch.equal(_bits(buf), _bits(at_launch * lb.world))


def test_without_hold_the_table_comes_back_on_its_own(dev):
    """hold=False is the double as it was: restored after the sleep whether or not anybody waited"""
    from permuto_sdf_amd import parallel
    g = torch.Generator().manual_seed(7)
    table = torch.randn(4096, generator=g).to(dev)
    orig = table.clone()
    with _loopback(hold=False) as lb:
        assert lb.hold is False and parallel.Loopback().hold is False
        su = parallel.ShardedUpdate()
        su.all_gather(table, (0, 2048))
        torch.cuda.synchronize()
        assert torch.equal(_bits(table), _bits(orig))
        buf = orig.clone()
        lb.all_reduce(buf)
        torch.cuda.synchronize()
        assert torch.equal(_bits(buf), _bits(orig * lb.world))


# ================================================================================================== the sampling phase
@pytest.mark.parametrize("start_iter", [1, 7])
@pytest.mark.parametrize("kind", ["manual", "masked", "autograd"])
def test_the_sampling_phase_reads_no_table_before_its_gather(dev, kind, start_iter):
    """`Trainer._samples` evaluates the SDF on the uniform samples and on the first round of importance samples; those values
    place the samples and are dropped again, so a NaN among them never reaches the loss.  They are counted here where they are
    made.  start_iter 7: the second step (iteration 8) also refreshes the occupancy grid from the SDF.

    On the trainer code before `_samples` waited for the SDF lattice's gather the two ManualTrainer variants fail here for any
    delay_cycles: every value of the first two evaluations is a NaN."""
    with _loopback():
        tr = _trainer(dev, kind, start_iter)
        reel = _reel(dev)
        tr.step(reel)
        assert sorted(tr._pending_gather) == [0, 1, 2], "all three parameter all-gathers should still be in flight"
        nans, sizes = [], []
        sdf_only = tr.sdf.sdf_only

        def counted(*a, **k):
            y = sdf_only(*a, **k)
            nans.append(torch.isnan(y).sum())     # a device tensor: no host sync inside the step
            sizes.append(y.shape[0])
            return y
        tr.sdf.sdf_only = counted
        try:
            loss = tr.step(reel)
        finally:
            del tr.sdf.sdf_only
        assert tr.last["nr_fg_samples"] > 0
        assert len(nans) >= (3 if start_iter == 7 else 2), len(nans)
        counts = [int(c) for c in nans]
        print("%s, second step at iteration %d: NaN per sdf_only call %s of %s values" % (kind, start_iter + 1, counts, sizes))
        assert counts == [0] * len(counts), (counts, sizes)
        tr.sync_parameters()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(p).all()) for p in tr.params)
        assert bool(torch.isfinite(loss))


# ================================================================================================== readers outside a step
@pytest.fixture()
def deferred(dev):
    """a trainer one deferred step in, its three gathers pending, under the held double"""
    with _loopback():
        tr = _trainer(dev, "manual", 1)
        reel = _reel(dev)
        tr.step(reel)
        assert sorted(tr._pending_gather) == [0, 1, 2]
        yield tr, reel


def test_a_checkpoint_saved_behind_a_deferred_step_holds_the_gathered_tables(dev, deferred, tmp_path):
    from permuto_sdf_amd.train_step import Trainer
    tr, _ = deferred
    tr.save_checkpoint(str(tmp_path))              # no sync_parameters(): the checkpoint waits for the gathers itself
    fresh = Trainer(dev, _hp())
    fresh.load_checkpoint(str(tmp_path))
    tr.sync_parameters()
    torch.cuda.synchronize()
    for name, a, b in zip(LATTICES, _tables(fresh), _tables(tr)):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(_bits(a), _bits(b)), name


def _centre_frame(dev, reel):
    """the smallest frame there is, 1 x 1, whose one ray is the optical axis of the reel's first camera: through the origin"""
    from permuto_sdf_amd import render
    K = torch.tensor([[72.0, 0.0, 0.5], [0.0, 72.0, 0.5], [0.0, 0.0, 1.0]], device=dev)
    return render.Frame(K, reel.tf_world_cam_reel[0], 1, 1)


def _finite(out, names):
    for k in names:
        v = getattr(out, k)
        assert v is not None and bool(torch.isfinite(v).all()), k


def test_render_waits_for_the_gathers(dev, deferred):
    from permuto_sdf_amd import render
    tr, reel = deferred
    out = render.FrameRenderer(tr).render(_centre_frame(dev, reel), camera_normals=True)
    assert not tr._pending_gather
    assert out.rgb.shape == (3, 1, 1)
    _finite(out, ("rgb", "rgb_bg", "normals", "normals_cam", "weights_sum"))


def test_render_traced_waits_for_the_gathers(dev, deferred):
    from permuto_sdf_amd import render
    tr, reel = deferred
    out = render.FrameRenderer(tr).render_traced(_centre_frame(dev, reel), camera_normals=True)
    assert not tr._pending_gather
    _finite(out, ("rgb", "normals", "normals_cam", "weights_sum", "depth"))


def test_render_views_waits_for_the_gathers(dev, deferred):
    from permuto_sdf_amd import render
    tr, reel = deferred
    views = render.FrameRenderer(tr).render_views([_centre_frame(dev, reel)])
    assert not tr._pending_gather
    assert views.shape == (1, 3, 1, 1) and bool(torch.isfinite(views).all())


def test_slice_waits_for_the_gathers(dev, deferred):
    from permuto_sdf_amd import render
    from permuto_sdf_amd.sdf_slice import SlicePlane
    tr, _ = deferred
    # one cell, at (-0.25, -0.25, 0.05): inside the unit box, so the SDF net is evaluated there
    out = render.FrameRenderer(tr).slice(SlicePlane(torch.eye(3), 0.05, extent_scale=0.25), size=1)
    assert not tr._pending_gather
    assert float(out.inside.sum()) == 1.0
    _finite(out, ("rgb", "sdf", "inside"))


# ================================================================================================== the writer
def test_a_step_that_reads_no_colour_lattice_still_retires_its_gather(dev):
    """No foreground samples (an empty occupancy grid, no refresh at iterations 3 and 4): the step never evaluates the colour
    network, so no READER waits for the colour lattice's gather -- the optimiser step, which writes the table, has to.  Before it
    did, the table was still NaN under hold when AdamW updated it, and stayed NaN."""
    with _loopback():
        tr = _trainer(dev, "manual", 3)
        tr.grid.set_grid_occupancy(torch.zeros_like(tr.grid.get_grid_occupancy()))
        reel = _reel(dev)
        losses = []
        for _ in range(2):
            losses.append(tr.step(reel))
            assert tr.last["nr_fg_samples"] == 0
            assert sorted(tr._pending_gather) == [0, 1, 2]
        tr.sync_parameters()
        torch.cuda.synchronize()
        for name, t in zip(LATTICES, _tables(tr)):
            assert bool(torch.isfinite(t).all()), name
        assert bool(torch.isfinite(torch.stack(losses)).all())


# ================================================================================================== early reductions
def _first_step(dev, serialize, hold):
    with _loopback(hold=hold, serialize=serialize) as lb:
        tr = _trainer(dev, "manual", 7, defer=not serialize)
        tr.capture_grads = {}
        loss = tr.step(_reel(dev))
        reduced = [g.clone() for g in tr.capture_grads["lattices_reduced"]]
        assert tr.last_dp and tr.last_dp["optimizer"] == "sharded"
        tr.sync_parameters()
        torch.cuda.synchronize()
        return reduced, float(loss), [k for k, _ in lb.launched]


def test_early_reductions_under_hold_equal_the_serialised_schedule(dev):
    """the first-step check of test_gpu_dp_schedule.py with the asynchronous run under hold: a lattice's reduction sums what its
    gradient buffer held when `_dp_lattice_final` started it, so a backward kernel that still added to the buffer afterwards
    would lose its contribution in every run.  The bar is that test's: 3 x what two serialised runs differ by (the float atomics
    of the lattice scatter), or 1e-5 of the reference's largest entry."""
    g_ref, _, _ = _first_step(dev, serialize=True, hold=False)
    g_ref2, _, _ = _first_step(dev, serialize=True, hold=False)
    g_got, loss, kinds = _first_step(dev, serialize=False, hold=True)
    assert loss == loss and abs(loss) != float("inf"), loss
    assert kinds.count("all_gather_params") == 3 and kinds.count("all_reduce") >= 3
    for k, (a, a2, b) in enumerate(zip(g_ref, g_ref2, g_got)):
        scale = float(a.abs().max())
        noise = float((a - a2).abs().max())
        err = float((a - b).abs().max())
        print("lattice %d: reduced gradient, held vs serialised %.2e, serialised vs itself %.2e (of a largest entry %.2e)"
              % (k, err, noise, scale))
        assert scale > 0 and err <= max(3.0 * noise, 1e-5 * scale), (k, err, noise, scale)
