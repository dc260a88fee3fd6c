"""CPU pin of the kNN tie order: line3dpp_amd/csrc/l3d_heap.h must pop exactly what std::priority_queue pops
(libstdc++, the container Line3D::matchingCPU keeps its kNN candidates in, line3D.cc:931-1007)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_heap_emulation_equals_std_priority_queue(tmp_path):
    exe = str(tmp_path / "heap_order")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "heap_order.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert "identical" in out.stdout


def test_division_free_depth_decision_equals_the_reference_arithmetic(tmp_path):
    """l3d_dev.h: depths_positive (stage 1 of the match kernel's candidate pipeline: the accept / reject decision of
    Line3D::triangulationDepths + line3D.cc:966-980 with one multiplication per depth, falling back to the division in
    the sliver where the two roundings could disagree) against exact_depths on 2.4 million cases incl. depths within a
    few ulp of L3D_EPS, degenerate denominators, NaN and inf -- and, since round 4, the FLOAT decision on 48-byte records
    (depths_positive32) on another 2.4 million cases incl. rays within 1e-5 .. 1e-8 of the other segment's plane,
    baselines within 1e-5 .. 1e-9 of a plane, camera centres six orders of magnitude apart, tiny baselines and NaN: whenever
    it reports `certain` it must equal exact_depths (uncertain candidates take the double-precision decision)."""
    exe = str(tmp_path / "depth_sign")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "cpp", "depth_sign.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert "identical" in out.stdout and " 0 mismatches" in out.stdout
    assert "float decision" in out.stdout and "0 mismatches among the certain" in out.stdout


def test_division_free_orientation_decision_equals_the_reference_arithmetic(tmp_path):
    """l3d_dev.h: orientation_ok_fast (checkMatchOrientation's keep / drop decision, line3D.cc:811-858 with
    View::segmentQualityAngle and unprojectSegment, as c^2 <= cos^2 * |v|^2 with a fallback to the reference's own
    arithmetic near the thresholds and for near-zero-length segments) against orientation_ok on 2.5 million cases incl.
    directions within a few ulp of both thresholds."""
    exe = str(tmp_path / "orient_sign")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "cpp", "orient_sign.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert "identical" in out.stdout and " 0 mismatches" in out.stdout


def test_prefilter_without_reciprocals_never_rejects_an_accepted_pair(tmp_path):
    """l3d_dev.h: prefilter_products (the fp32 pre-filter of k_match_pairs in its form without v_rcp_f32) against the
    reference's arithmetic (exact_overlap = Line3D::matchingCPU line3D.cc:919-958 + mutualOverlap :1086-1165): on 61
    million (pair, threshold) cases -- random, along the epipolar band, nearly parallel to the pencil, end points on an
    epipolar line, thresholds up to the pair's own overlap -- no pair with overlap > threshold is rejected."""
    exe = str(tmp_path / "prefilter_cover")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "cpp", "prefilter_cover.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert "covered" in out.stdout and " 0 lost" in out.stdout


def test_affinity_similarity_form_and_symmetry(tmp_path):
    """l3d_dev.h: sim_affinity (k_affinity.hip takes ONE exponential, of the minimum of the five arguments) against the
    literal form of Line3D::similarity (line3D.cc:1467-1553: five exponentials, then the fmin chain), bit for bit, and
    sim(h1, h2) == sim(h2, h1) bit for bit, on 3.2 million random and forced hypotheses: lengths below L3D_EPS, float dot
    products above 1 (the clamp), exactly 90 degrees, depths at the cutoff, med_scene_depth_lines at 0 and around L3D_EPS,
    regularisers of 0 (NaN at distance 0, -inf beyond), all four position terms NaN."""
    exe = str(tmp_path / "sim_affinity")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "cpp", "sim_affinity.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert "identical, 0 mismatches" in out.stdout and "symmetric, 0 asymmetric" in out.stdout
    assert "an arm was not reached" not in out.stdout


def test_scoring_similarity_at_its_thresholds(tmp_path):
    """l3d_dev.h: sim_decide / sim_far / sim_value / window_sq / support_radius / dir_decide32 / sim_thresholds (the
    decision of phase B, `similarityForScoring(i, j) > 0.5`, taken as comparisons with bisected thresholds inside padded
    depth windows, the angle in fp32 away from its thresholds) against a literal restatement of line3D.cc:1417-1446 and
    :1571-1583 with libm's expf, acos and fmin.  Every float within 2^16 ulp of y_thr, x_hi, x_lo, 0 and +-1 for nine
    sigma_a on both sides of the switch to the x_hi == 0 form (no flip back: the bisection's monotonicity); 6 million tuples
    forced to within 3 ulp of a threshold in any component, with NaN, -inf, denormal, infinite and overflowing terms, zero
    lengths and clamped dot products; the early-out over every float exponent of reg; the windows against the farthest
    depth the reference accepts; the fp32 angle on unprojected directions within 1e-5 of a threshold; the value within one
    ulp.  The pin prints the three measured numbers: the largest |xf - x|, the smallest window ratio, the one-ulp count."""
    exe = str(tmp_path / "sim_scoring")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "cpp", "sim_scoring.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert "identical, 0 mismatches" in out.stdout
    assert "an arm was not reached" not in out.stdout and "not reached" not in out.stdout
    assert "0 outside" in out.stdout and "0 of those wrong" in out.stdout and "0 accepted by the reference" in out.stdout
