"""Where the bound of the GPU sanity check (tests/test_gpu_project.py::test_context_sanity_of_the_residuals) comes from:
the numpy model of DESIGN §16 on the final lines THE REFERENCE'S OWN CODE (oracle/_ref) reconstructs from the golden
scene.  The 95 % visibility is a condition the scene has to meet, and the median end point distance is the figure the
GPU test doubles.  CPU only; skipped where oracle/_ref has not been built."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import project_lines_cases as Cs
from tests import project_lines_model as M

pytestmark = pytest.mark.skipif(not O.have_reference(), reason="oracle/_ref not built (needs the reference's sources)")


def test_reference_lines_meet_the_sanity_condition_and_give_the_cpu_median():
    from tests.golden.make_golden import golden_scene
    sc = golden_scene()
    r = O.Oracle(reference=True)
    r.add_scene(sc)
    r.match_images()
    r.reconstruct(3)
    lines = r.lines()
    assert len(lines) > 20
    P1 = np.concatenate([L["collinear3Dsegments"][:, 0:3] for L in lines])
    P2 = np.concatenate([L["collinear3Dsegments"][:, 3:6] for L in lines])
    line = np.concatenate([[i] * len(L["collinear3Dsegments"]) for i, L in enumerate(lines)]).astype(np.uint32)
    cams = [dict(K=v.K, R=v.R, t=np.asarray(v.t, np.float64).reshape(3), width=v.width, height=v.height) for v in sc.views]
    rec = M.project_segments(cams, P1, P2, line)
    n_pairs = sum(len(L["residuals"]) for L in lines)
    frac, median = Cs.residual_sanity(lines, rec, [v.cam for v in sc.views], {v.cam: v.segs for v in sc.views})
    print(f"{len(lines)} lines, {n_pairs} (line, residual) pairs: visible {100 * frac:.1f} %, median end point distance {median:.5f} px")
    assert frac >= Cs.SANITY_MIN_VISIBLE, "the golden scene does not meet the condition of the sanity check: choose another"
    # the constant the GPU test doubles is this figure, to the five digits it is written with
    assert abs(median - Cs.SANITY_CPU_MEDIAN_PX) <= 5e-6
