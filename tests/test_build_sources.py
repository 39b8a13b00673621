"""The build list names every translation unit in csrc/, and the stale-header check watches
every header they include (a header it misses would leave objects stale after an edit)."""

import os
import re

from lasp_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def test_sources_are_the_translation_units_present():
    present = {f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp"))}
    assert len(build.SOURCES) == len(set(build.SOURCES))
    assert set(build.SOURCES) == present


def test_every_quoted_include_is_watched():
    watched = {os.path.realpath(h) for h in build.headers()}
    seen = 0
    for f in sorted(os.listdir(build.CSRC)):
        if not f.endswith((".hip", ".cpp", ".h")):
            continue
        for inc in INCLUDE.findall(open(os.path.join(build.CSRC, f)).read()):
            path = os.path.realpath(os.path.join(build.CSRC, inc))
            assert os.path.isfile(path), f"{f} includes {inc}, which does not resolve"
            assert path in watched, f"{f} includes {inc}, which the stale check does not watch"
            seen += 1
    assert seen >= len(build.SOURCES)
