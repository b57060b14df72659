"""The kernel sources test two experiment macros and no others: MI_WIN_STAMPS and MI_FOLD_STAMPS, the in-kernel clock
stamps.  Every other knob is a constexpr value with its measurement in EXPERIMENTS.md ("Decided knobs"),
so the kernel in front of a reader is the kernel that runs.  A new experiment macro has to be added to ALLOWED on purpose.
Host-only: reads the sources."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "optimization_amd", "csrc")
ALLOWED = {"MI_WIN_STAMPS", "MI_FOLD_STAMPS"}
CONDITIONAL = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$")


def conditionals(text):
    """the expression of every #if / #ifdef / #ifndef / #elif, continuation lines joined, comments dropped"""
    text = re.sub(r"\\\n", " ", text)
    for line in text.split("\n"):
        m = CONDITIONAL.match(line)
        if m:
            yield re.sub(r"//.*|/\*.*?\*/", " ", m.group(1))


def test_only_the_stamp_macros_are_tested_by_the_preprocessor():
    files = sorted(f for f in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(f))
    assert len(files) > 20 and os.path.join(CSRC, "stiefel_wide.h") in files, files
    found = {}
    for f in files:
        with open(f, errors="replace") as fh:
            for expr in conditionals(fh.read()):
                for name in re.findall(r"\bMI_[A-Za-z0-9_]+", expr):
                    found.setdefault(name, set()).add(os.path.basename(f))
    assert set(found) == ALLOWED, {n: sorted(w) for n, w in found.items() if n not in ALLOWED} or sorted(ALLOWED - set(found))
