"""INTEGRATION.md's Environment table names exactly the environment variables
the sources read, and the C++ reads them in the two env.h headers only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "band_amd", "csrc")
ENV_HEADERS = {os.path.join("backend", "hip", "env.h"), os.path.join("engine", "env.h")}


def csrc_sources():
    for dirpath, dirs, files in os.walk(CSRC):
        dirs[:] = [d for d in dirs if not d.startswith("build")]
        for f in files:
            if f.endswith((".cc", ".h", ".hip", ".hpp")):
                path = os.path.join(dirpath, f)
                yield os.path.relpath(path, CSRC), open(path).read()


def test_getenv_only_in_env_headers():
    users = {rel for rel, src in csrc_sources() if "getenv" in src}
    assert users == ENV_HEADERS
    assert not any(rel.startswith("kernels") for rel in users)


def test_environment_table_matches_sources():
    read = set()
    for rel, src in csrc_sources():
        if rel in ENV_HEADERS:
            # every getenv there takes a helper's `name`; the readers pass literals
            assert set(re.findall(r"getenv\(([^)]*)\)", src)) == {"name"}, rel
            read |= set(re.findall(r'\b(?:Flag|Int|Str)\("([A-Z][A-Z0-9_]*)"', src))
    for path in glob.glob(os.path.join(ROOT, "band_amd", "*.py")):
        read |= set(re.findall(r'environ(?:\.get\(|\[)\s*"([A-Z][A-Z0-9_]*)"', open(path).read()))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc[doc.index("## 7. Environment"):]
    table = set(re.findall(r"^\| `([A-Z][A-Z0-9_]*)` \|", section, flags=re.M))
    assert len(read) > 15
    assert table == read, (sorted(table - read), sorted(read - table))
