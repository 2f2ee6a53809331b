"""How the tests build and run a stand-alone program over a host twin of the k-mer index (tests/*_asan.cpp, tests/khost_program.hpp): with
the sanitizers compiled into the program itself.  Nothing loaded into Python is sanitised."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soapdenovo2_amd", "csrc")


def build_and_run(tmp_path, program, sources, ok_lines):
    """tests/<program>.cpp with csrc/<source> for every source, under -fsanitize=address,undefined: it must build, exit 0 and print every
    one of ok_lines."""
    exe = str(tmp_path / program)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + CSRC, os.path.join(ROOT, "tests", program + ".cpp")] + [os.path.join(CSRC, s) for s in sources] + ["-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and all(line in ran.stdout for line in ok_lines), ran.stdout + ran.stderr
