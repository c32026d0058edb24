"""Builds scripts/apng_parse_sanitize.cpp — the APNG decoder's host-side chunk walk as a stand-alone program — with
-fsanitize=address,undefined and runs it on every fixture of tests/apng_cases.py (good, corrupt, malformed,
unsupported), each whole and truncated at every byte offset (a fixture above 16 KiB, such as the one of 65536 frames: at
every offset of its first and last 4096 bytes).  Host only: no GPU, nothing loaded into Python.

    python scripts/apng_parse_sanitize.py

Prints the program's counts; any sanitizer report ends it with a non-zero status."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import apng_cases as cases  # noqa: E402


def main():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    fx = cases.fixtures()
    files = dict(fx["good"])
    for kind in ("malformed", "unsupported", "corrupt"):
        files.update({"%s_%s" % (kind, k): v[0] for k, v in fx[kind].items()})
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "apng_parse_sanitize")
        subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", os.path.join(ROOT, "scripts", "apng_parse_sanitize.cpp"), "-o", exe])
        paths = []
        for k, (name, data) in enumerate(sorted(files.items())):
            paths.append(os.path.join(tmp, "%03d_%s.png" % (k, name.replace("/", "_"))))
            with open(paths[-1], "wb") as fh:
                fh.write(data)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        rc = subprocess.call([exe] + paths, env=env)
    print("apng_parse_sanitize: %d fixtures, exit status %d" % (len(paths), rc))
    return rc


if __name__ == "__main__":
    sys.exit(main())
