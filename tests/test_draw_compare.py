"""dm_draw_compare (include/eslam_detmath.h): the integer decision of "stratified draw <= target"
that K3's draw counting takes instead of evaluating the draws, against the draws' definition
(tests/c/check_draw_cmp.c: the cases, the checks and the expected number of ambiguous random
targets are in its header)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_draw_compare_against_definition(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("checkdrawcmp") / "check_draw_cmp")
    subprocess.run(["gcc", "-O2", "-std=c11", "-mfma", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "check_draw_cmp.c"), "-o", exe], check=True)
    out = subprocess.run([exe, "1500"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 wrong decisions" in out.stdout
    assert " 0 bound violations" in out.stdout
    assert " 0 random ambiguous" in out.stdout
    assert " 0 domain failures" in out.stdout
    m = re.search(r"(\d+) certain, (\d+) ambiguous.*?(\d+) random targets", out.stdout)
    certain, ambiguous, random_targets = (int(g) for g in m.groups())
    # both kinds of answer occur, and every random target was decided
    assert ambiguous > 0 and certain >= random_targets > 0
