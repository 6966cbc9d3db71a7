"""The four plan transforms at their identities -- `take(p, arange(B))`, `shift(p, 0)`, `delay(p, 0)`, `concat([p])` -- on the GPU: each
returns a rows-free RaggedBatch that is the source plan again, bit for bit, in every array it carries, and whose sampled rows are the
source's rows.  What one derived batch holds is thereby pinned for all of them at once, whichever code assembles it.

Three sources, all at dt = 0.05: a uniform Plan (B = 3, m = 2), a ragged batch (1, 3 and 2 segments, one cruise speed per mission), and
the RaggedPlan that `plan_collision_free` returns without obstacles (B = 2), which the transforms read through its batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT, COUNTS, SPEEDS = 0.05, (1, 3, 2), (2.0, 3.0, 2.5)
SOURCES = ("uniform", "ragged", "collision_free")
TRANSFORMS = ("take", "shift", "delay", "concat")


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


_CACHE = {}


def case(eng):
    """Computed once and left unchanged: the three sources, with rows."""
    if not _CACHE:
        from oracle import minsnap_oracle as mo
        wps = mo.synthetic_missions(3, 3)
        _CACHE.update(uniform=eng.plan(mo.synthetic_missions(3, 2), 3.0, DT),
                      ragged=eng.plan_ragged([wps[b][:c + 1] for b, c in enumerate(COUNTS)], np.array(SPEEDS), DT),
                      collision_free=eng.plan_collision_free(mo.synthetic_missions(2, 3), None, 3.0, DT))
    return _CACHE


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64 if a.dtype == np.float64 else a.dtype),
                                                                        b.view(np.int64 if b.dtype == np.float64 else b.dtype))


def transformed(eng, how, p):
    import torch
    B = int(p.B)
    if how == "take":
        return eng.take(p, np.arange(B))
    if how == "shift":
        return eng.shift(p, torch.zeros((B, 3), dtype=torch.float64))
    if how == "delay":
        return eng.delay(p, torch.zeros((B,), dtype=torch.int32))
    return eng.concat([p])


@pytest.mark.parametrize("which", SOURCES)
def test_the_identity_transforms_give_the_source_again(eng, which):
    import torch
    from uav_ac.fleet import RaggedBatch
    p = case(eng)[which]
    src = p.batch if which == "collision_free" else p         # (the transforms read a RaggedPlan through its batch)
    B = int(src.B)
    ragged = hasattr(src, "seg_offsets")
    m = int(src.max_m if ragged else src.m)
    so = np.asarray(src.seg_offsets_host, dtype=np.int64) if ragged else np.arange(B + 1, dtype=np.int64) * m
    want = dict(coeffs=src.coeffs.cpu().numpy().reshape(-1, 8, 3), times=src.times.cpu().numpy().reshape(-1),
                seg_rows=src.seg_rows.cpu().numpy().reshape(-1), seg_offsets=so, row_offsets=src.row_offsets.cpu().numpy(),
                first_yaw=src.first_yaw.cpu().numpy())
    rows = p.traj.cpu().numpy()
    assert want["coeffs"].shape[0] == so[-1] and rows.shape == (int(src.total_rows), 11) and rows.shape[0] > B
    for how in TRANSFORMS:
        out = transformed(eng, how, p)
        torch.cuda.synchronize()
        assert isinstance(out, RaggedBatch), how
        assert out.free_times is True and out.waypoints is None and out.traj is None, how
        assert out.B == B and out.max_m == (m + 1 if how == "delay" else m), how
        assert out.total_rows == int(src.total_rows) and out.dt == float(src.dt) == DT, how
        assert out.seg_offsets.dtype == torch.int64 and out.seg_offsets.device == eng.device, how
        assert same_bits(np.asarray(out.seg_offsets_host), so), how
        for name, ref in want.items():
            assert same_bits(getattr(out, name).cpu().numpy(), ref), (how, name)
        eng.sample_rows(out)
        torch.cuda.synchronize()
        assert out.traj is not None and same_bits(out.traj.cpu().numpy(), rows), how
        assert same_bits(out.first_yaw.cpu().numpy(), want["first_yaw"]), how      # (the sampler writes the headings again: the same ones)
