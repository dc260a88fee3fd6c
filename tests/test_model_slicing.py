"""CPU pin of the slicing rule that the comparison and the merge (§19) share: slice_plan of
line3dpp_amd/csrc/l3d_model.h.  Both kernels rely on its invariants -- no slice is empty, every chunk of references is
covered, the per-(query, slice) cells stay within the budget -- and the hand-worked pins keep the rule what it was when
each stage had a copy of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slice_plan_invariants_and_pins(tmp_path):
    exe = str(tmp_path / "model_slicing")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "model_slicing.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert "identical" in out.stdout
