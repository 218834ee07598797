"""The M355_* environment switches are a declared interface: csrc/switches.hip is the only file of the native library that
reads the environment, and tools/README.md lists every switch with its lifetime.  A new switch that is read with a stray
getenv, or that is not in the table, fails here.  Host only: text of the tree, no library, no GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "defectdetection_viaobjectdetection_amd", "csrc")
NAME = r"M355_[A-Z0-9_]+"


def read(*parts):
    with open(os.path.join(*parts), encoding="utf-8", errors="replace") as f:
        return f.read()


def first_column(part):
    return [m for line in part.splitlines() if line.startswith("| `") for m in re.findall(NAME, line.split("|")[1])]


def readme_tables():
    """Names in the first column of the two switch tables of tools/README.md: (native library, Python side), as lists."""
    text = read(ROOT, "tools", "README.md")
    native, python = text.split("## Switches of the native library", 1)[1].split("### Switches read by the Python package", 1)
    return first_column(native), first_column(python.split("\n## ", 1)[0])


def test_only_switches_hip_reads_the_environment():
    sources = [f for f in sorted(os.listdir(CSRC)) if not f.endswith(".o")]   # (objects of an in-tree build lie beside them)
    stray = [f for f in sources if f != "switches.hip" and "getenv" in read(CSRC, f)]
    assert not stray, stray
    assert "getenv" in read(CSRC, "switches.hip")


def test_readme_table_lists_exactly_the_switches_of_switches_hip():
    in_code = set(re.findall(r'"(%s)"' % NAME, read(CSRC, "switches.hip")))
    native, _ = readme_tables()
    assert len(in_code) > 60, len(in_code)
    assert len(native) == len(set(native)), "listed twice: %s" % sorted(n for n in set(native) if native.count(n) > 1)
    assert set(native) == in_code, (sorted(in_code - set(native)), sorted(set(native) - in_code))


def test_every_switch_the_tests_tools_and_bench_use_is_documented():
    native, python = readme_tables()
    known = set(native) | set(python)
    files = [os.path.join(ROOT, "bench.py")]
    for top in ("tests", "tools"):
        for d, _, names in os.walk(os.path.join(ROOT, top)):
            files += [os.path.join(d, n) for n in names if n.endswith((".py", ".sh"))]
    unknown = {}
    for path in files:
        for name in set(re.findall(NAME, read(path))):
            if not name.startswith("M355_ERR_") and name not in known:
                unknown.setdefault(name, []).append(os.path.relpath(path, ROOT))
    assert not unknown, unknown
