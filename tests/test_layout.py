"""The suite's layout: what test files share lives in the support modules (tests/gpu_support.py,
tests/abi_support.py, tests/fast_scenes.py, ...), never in another test file, so that editing one
file's tests cannot break another's."""
import ast
import glob
import os


def test_no_test_module_imports_another():
    here = os.path.dirname(os.path.abspath(__file__))
    offenders = []
    for path in sorted(glob.glob(os.path.join(here, "test_*.py"))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""] + [a.name for a in node.names]  # from tests import test_x
            else:
                continue
            offenders += ["%s:%d imports %s" % (os.path.basename(path), node.lineno, n) for n in names
                          if n.split(".")[-1].startswith("test_")]
    assert not offenders, offenders
