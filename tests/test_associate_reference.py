"""Where the condition of the GPU sanity check (tests/test_gpu_associate.py::test_context_sanity_of_the_residuals) comes
from: the numpy model of DESIGN §17 on the final lines THE REFERENCE'S OWN CODE (oracle/_ref) reconstructs from the golden
scene, with the default thresholds (2.5 px, 10 degrees, 0.5).  CPU only; skipped where oracle/_ref has not been built."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import associate_cases as Cs
from tests import associate_model as A
from tests import project_lines_model as M

pytestmark = pytest.mark.skipif(not O.have_reference(), reason="oracle/_ref not built (needs the reference's sources)")


def test_reference_lines_own_their_residuals():
    from tests.golden.make_golden import golden_scene
    sc = golden_scene()
    r = O.Oracle(reference=True)
    r.add_scene(sc)
    r.match_images()
    r.reconstruct(3)
    lines = r.lines()
    P1 = np.concatenate([L["collinear3Dsegments"][:, 0:3] for L in lines])
    P2 = np.concatenate([L["collinear3Dsegments"][:, 3:6] for L in lines])
    line = np.concatenate([[i] * len(L["collinear3Dsegments"]) for i, L in enumerate(lines)]).astype(np.uint32)
    cams = [dict(K=v.K, R=v.R, t=np.asarray(v.t, np.float64).reshape(3), width=v.width, height=v.height) for v in sc.views]
    rec = M.project_segments(cams, P1, P2, line)
    assoc = {v.cam: A.associate(rec[k], v.segs, **Cs.DEFAULTS) for k, v in enumerate(sc.views)}
    pairs, own, other, none, _ = Cs.residual_ownership(lines, assoc)
    in_cluster = {(int(res[0]), int(res[1])) for L in lines for res in L["residuals"]}
    new = sum(int(a["record"][s] >= 0) for cam, a in assoc.items() for s in range(len(a)) if (cam, s) not in in_cluster)
    outside = sum(len(a) for a in assoc.values()) - len(in_cluster)
    ambiguous = sum(int((a["n_accepted"] > 1).sum()) for a in assoc.values())
    print(f"{len(lines)} lines, {pairs} (line, residual) pairs: {own} on their own line, {other} on another, {none} on none; "
          f"{new} of the {outside} segments in no cluster are assigned; {ambiguous} ambiguous segments")
    assert (pairs, own, other) == (Cs.REFERENCE_PAIRS, Cs.REFERENCE_OWN, Cs.REFERENCE_OTHER)
    # the condition the GPU sanity check uses
    assert own / pairs >= Cs.SANITY_MIN_OWN_SHARE and other == 0
    assert ambiguous == 0
    # with 5 px / 0.25 the tie rule is reachable on real data
    loose = dict(Cs.DEFAULTS, max_distance=5.0, min_overlap=0.25)
    n_loose = sum(int((A.associate(rec[k], v.segs, **loose)["n_accepted"] > 1).sum()) for k, v in enumerate(sc.views))
    print(f"5 px / 0.25: {n_loose} ambiguous segments")
    assert n_loose > 0
