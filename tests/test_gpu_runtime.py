"""One HIP runtime per process: a Weaver created before `import torch` must
leave torch's GPU usable (abi._share_torch_hip_runtime), and both see one
libamdhip64 mapping.  And the options of a live context (cw_ctx_set_option):
they take effect on the next call, whatever the context cached for the layout."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from cause_amd import abi, gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
import re
from cause_amd import abi
w = abi.Weaver(0)
import torch
assert torch.cuda.is_available(), "torch lost the GPU"
maps = set(re.findall(r"\S*libamdhip64\S*", open("/proc/self/maps").read()))
assert len(maps) == 1, maps
x = torch.arange(10, device="cuda")
w.set_stream(torch.cuda.current_stream().cuda_stream)
w.set_stream(None)
w.close()
print("ok", int(x.sum()))
"""


def test_weaver_first_then_torch_share_one_runtime():
    p = subprocess.run([sys.executable, "-c", PROG], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "ok 45" in p.stdout


# ---------------------------------------------------------------- options ----
SPEC = dataclasses.replace(gen.CONFIG2, nodes_per_doc=3000)


def _batch(first, n_docs):
    """(inputs, the oracle's weave of them): documents first .. first + n_docs."""
    off, idk, ck, kd = gen.generate(SPEC, first, first + n_docs)
    perm, vis, st = oracle.batch_lists(off, idk, ck, kd, method=oracle.METHOD_EFF)
    assert not st.any()
    return (off, idk, ck, kd), (perm, vis)


@pytest.fixture(scope="module")
def batch():
    return _batch(0, 5)


@pytest.fixture(scope="module")
def one_doc():
    return _batch(7, 1)


def _weave_equals_oracle(w, inputs, ref):
    res = w.weave_lists(*inputs, SPEC.layout(), yarns=False)
    assert not res.status.any(), res.status
    assert np.array_equal(res.weave_perm, ref[0])
    assert np.array_equal(res.visible(), ref[1])
    return res


def test_options_change_the_path_of_a_cached_layout(batch):
    """One context, one batch, four calls: every call is the oracle's weave and
    runs the kernels of the options set just before it, although the document
    tables (and the map packs) are cached by the layout, which never changes."""
    inputs, ref = batch
    defaults = {"tour": 1, "fused": 1, "tour_log2k": 3}
    steps = [({}, {"weave"}, {"walk"}),
             ({"tour": 0}, {"walk", "rank", "emit"}, {"weave", "tour"}),
             ({"tour": 1, "fused": 0, "tour_log2k": 7}, {"front", "tree", "tour"}, {"weave", "walk"}),
             (defaults, {"weave"}, {"walk", "front", "tour"})]
    with abi.Weaver(0) as w:
        w.set_profiling(True)
        for options, ran, not_ran in steps:
            for name, value in options.items():
                w.set_option(name, value)
            w.reset_kernel_stats()
            _weave_equals_oracle(w, inputs, ref)
            stats = set(w.kernel_stats())
            assert ran <= stats and not (not_ran & stats), (options, sorted(stats))


PHASE_LINES = ("weave phases", "front phases", "tree phases", "tour phases")


def test_phase_stamps_do_not_change_the_weave(batch, capfd):
    """tree_prof = 1 on every path that stamps phases: the weave is the oracle's
    and each kernel that ran reports its phases once on stderr.  Documents of
    3,001 nodes: two of k_tree_l's 2,048-rank tiles, three of k_tree's.  (tour
    = 0 leaves the front end as it is, so k_front reports next to the tree.)"""
    from tests.test_gpu_maps import check as check_maps

    inputs, ref = batch
    assert int(np.diff(inputs[0]).max()) > 2048
    cases = [({"tree_prof": 1}, {"weave phases"}),
             ({"tree_prof": 1, "fused": 0}, {"front phases", "tree phases", "tour phases"}),
             ({"tree_prof": 1, "tour": 0}, {"front phases", "tree phases"}),
             ({"tree_prof": 1, "tree_l": 0, "fused": 0}, {"front phases", "tree phases", "tour phases"})]
    for options, lines in cases:
        with abi.Weaver(0, options=options) as w:
            capfd.readouterr()
            _weave_equals_oracle(w, inputs, ref)
        err = capfd.readouterr().err
        assert {ln for ln in PHASE_LINES if ln in err} == lines, (options, err)
        assert all(err.count(ln) == 1 for ln in lines), (options, err)

    spec = gen.MapSpec(nodes_per_coll=60, seed=13)
    off, idk, ck, ci, kd = gen.generate_maps(spec, 0, 40, nthreads=1)
    with abi.Weaver(0, options={"tree_prof": 1}) as w:
        capfd.readouterr()
        check_maps(w, off, idk, ck, ci, kd, spec.layout()[1])
    err = capfd.readouterr().err
    assert err.count("map pack phases") == 1, err


def _walk_with_4_entry_slots(w, one_doc):
    """giant_log2cap = 0 is clamped to 2 (4-entry walk slots): the giant path's
    splitter blocks of 8 nodes then overflow their slots."""
    w.set_option("giant_min", 0)
    w.set_option("giant_log2cap", 0)
    _weave_equals_oracle(w, *one_doc)
    assert w.counter("continued_sublists") > 0


def test_option_errors_and_clamping(batch, one_doc):
    with abi.Weaver(0) as w:
        with pytest.raises(abi.WeaveError, match="unknown option no_such_option"):
            w.set_option("no_such_option", 1)
        _weave_equals_oracle(w, *batch)  # the context still weaves
        _walk_with_4_entry_slots(w, one_doc)
    with pytest.raises(abi.WeaveError, match="unknown option"):
        abi.Weaver(0, options={"CW_TOUR": 0})


def test_counter_is_of_the_last_call(batch, one_doc):
    """cw_get_counter after a call that does not walk in HBM reports 0, not the
    count an earlier walk left."""
    with abi.Weaver(0) as w:
        _walk_with_4_entry_slots(w, one_doc)
        w.set_option("giant_min", 1 << 16)
        w.set_option("giant_log2cap", 5)
        w.set_profiling(True)
        _weave_equals_oracle(w, *batch)
        assert "weave" in w.kernel_stats()  # the fused kernel: no HBM walk
        assert w.counter("continued_sublists") == 0
