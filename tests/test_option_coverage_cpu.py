"""include/dfe.h promises for the launchers' behaviour switches that "every choice has a parity test or is a pure scheduling choice".
This keeps the promise checkable: every key of dfe_opt_names (csrc/dfe_ctx.hip), and "graphs", is forced by name in at least one
tests/test_gpu_*.py -- as an argument of ctx.set_option(...), ctx.options(...) or a module's _opt(...) helper.  A key that reaches such a
call only through a variable or a dict does not count: the next reader must be able to find the test by searching for the key."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# keys without a test that forces them, and why: nothing else may be listed
EXEMPT = {"debug_arena": "only prints where the scratch arena landed (stderr); no launcher reads it"}


def option_keys():
    src = open(os.path.join(ROOT, "depth-estimation_amd", "csrc", "dfe_ctx.hip")).read()
    table = re.search(r"dfe_opt_names\[DFE_NOPT\]\s*=\s*\{(.*?)\n\};", src, re.S)
    assert table, "dfe_opt_names not found in csrc/dfe_ctx.hip"
    keys = re.findall(r'\{\s*"(\w+)"\s*,\s*"DFE_\w+"\s*,\s*(?:true|false)\s*\}', table.group(1))
    assert len(keys) == len(set(keys)) and len(keys) >= 27
    return keys + ["graphs"]


def forcing_calls(text):
    """the argument text of every set_option( / options( / _opt( call in `text` (balanced parentheses; the suite's calls hold no parenthesis in a string)"""
    for m in re.finditer(r"\b(?:set_option|options|_opt)\(", text):
        depth, i = 1, m.end()
        while i < len(text) and depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        yield text[m.end() : i - 1]


def forced_keys():
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))):
        for args in forcing_calls(open(path).read()):
            for k in re.findall(r"""["'](\w+)["']""", args) + re.findall(r"\b(\w+)\s*=(?!=)", args):
                found.setdefault(k, set()).add(os.path.basename(path))
    return found


def test_option_table_matches_the_python_keys():
    from depth_estimation_amd._lib import OPTION_KEYS

    assert sorted(option_keys()) == sorted(OPTION_KEYS)


def test_every_option_key_is_forced_by_a_gpu_test():
    keys, found = option_keys(), forced_keys()
    assert set(EXEMPT) == {"debug_arena"} and set(EXEMPT) <= set(keys)
    missing = [k for k in keys if k not in found and k not in EXEMPT]
    assert not missing, "no tests/test_gpu_*.py forces %s through set_option( / options( / _opt(" % ", ".join(missing)
    for k in EXEMPT:
        assert k not in found, "%s is forced by %s: take it off the exemption list" % (k, sorted(found[k]))


def test_the_scan_sees_each_spelling_and_nothing_else():
    text = 'ctx.set_option("a_key", 1)\nwith ctx.options(b_key=0, c_key=f(x)):\n_opt(dfe, "d_key", "1")\nctx.set_option(key, v)\nd = {"e_key": 0}\nctx.options(**d)\nif g_key == 1: pass\n'
    got = set()
    for args in forcing_calls(text):
        got.update(re.findall(r"""["'](\w+)["']""", args) + re.findall(r"\b(\w+)\s*=(?!=)", args))
    assert {k for k in got if k.endswith("_key")} == {"a_key", "b_key", "c_key", "d_key"}
