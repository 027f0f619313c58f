"""`make san_check` whole (no GPU): every stand-alone host program of the target, built with the Makefile's
SANFLAGS (ASan + UBSan on the host objects; nothing is preloaded, each program has its own main) and run.
The programs are taken from the target's own recipe, so one added there runs here too."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "generalsparse_amd", "csrc")
PROGRAMS = ("convert_values_check", "sddmm_layout_check", "gather_layout_check", "value_map_check")


def test_every_program_of_san_check():
    dry = subprocess.run(["make", "-n", "-B", "-C", CSRC, "san_check"], capture_output=True, text=True, check=True).stdout
    ran = re.findall(r"^\./build_san/(\w+)$", dry, re.M)
    assert sorted(ran) == sorted(PROGRAMS), ran
    for name in ran:
        link = [ln for ln in dry.splitlines() if f"-o build_san/{name} " in ln]
        assert link and "-fsanitize=address,undefined" in link[0], (name, link)
    jobs = str(min(16, os.cpu_count() or 8))
    subprocess.run(["make", "-s", "-j", jobs, "-C", CSRC] + [f"build_san/{n}" for n in ran], check=True)
    for name in ran:
        run = subprocess.run([os.path.join(CSRC, "build_san", name)], capture_output=True, text=True)
        assert run.returncode == 0, (name, run.stdout[-2000:] + run.stderr[-2000:])
        if name == "gather_layout_check":
            m = re.search(r"gather_layout_check: (\d+) arrays, (\d+) failures", run.stdout)
            assert m and int(m.group(1)) >= 163 and int(m.group(2)) == 0, run.stdout + run.stderr[-2000:]
    # the target itself: the same programs, in its order, nothing left to build
    whole = subprocess.run(["make", "-s", "-C", CSRC, "san_check"], capture_output=True, text=True)
    assert whole.returncode == 0, whole.stdout[-2000:] + whole.stderr[-2000:]
