"""The environment variables the library reads are exactly the ones INTEGRATION.md lists (host-only)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mecano_amd", "csrc")


def read_in_sources():
    names = set()
    for name in os.listdir(CSRC):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            names |= set(re.findall(r'getenv\("(MH_[A-Z0-9_]+)"\)', f.read()))
    return names


def listed_in_integration():
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as f:
        text = f.read()
    section = text.split("## 5. Environment variables the library reads", 1)[1].split("\n## ", 1)[0]
    rows = re.findall(r"^\| `(MH_[A-Z0-9_]+)` \|[^|]*\| (user setting|test / measurement switch) \|$", section, re.M)
    names = [n for n, _ in rows]
    assert len(names) == len(set(names)), "a variable is listed twice"
    return set(names)


def test_every_environment_variable_is_listed():
    read, listed = read_in_sources(), listed_in_integration()
    assert read, "no getenv(\"MH_...\") found: the pattern no longer matches the sources"
    assert read - listed == set(), "read by the library but not listed in INTEGRATION.md section 5"
    assert listed - read == set(), "listed in INTEGRATION.md section 5 but no longer read by the library"
