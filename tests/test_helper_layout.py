"""Where the suite's helpers live: tests import helper modules, helper modules never hold tests, and no file imports a
test file.  Every tests/*.py and tools/*.py is parsed, none is run.  (A test that starts a child process to run its own file's test
functions under another environment names that file in the child's program text; that is not an import between test files and is
not looked for here.)"""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))


def parsed(path):
    with open(path) as fh:
        return ast.parse(fh.read(), path)


def imported_modules(tree, package):
    """every module an import statement anywhere in the file names, relative ones resolved against `package`"""
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                yield a.name
        elif isinstance(node, ast.ImportFrom):
            base = (package if node.level else "") + ("." if node.level and node.module else "") + (node.module or "")
            yield base
            for a in node.names:
                yield base + "." + a.name


def test_no_file_imports_a_test_file():
    assert len(FILES) > 60, len(FILES)
    bad = []
    for path in FILES:
        package = os.path.basename(os.path.dirname(path))
        for name in imported_modules(parsed(path), package):
            parts = name.split(".")
            if parts[0] == "tests" and any(p.startswith("test_") for p in parts[1:2]):
                bad.append((os.path.relpath(path, ROOT), name))
    assert not bad, bad


def test_helper_modules_define_no_tests():
    bad = []
    for path in FILES:
        if os.path.basename(path).startswith("test_"):
            continue
        for node in ast.walk(parsed(path)):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and node.name.startswith("test_"):
                bad.append((os.path.relpath(path, ROOT), node.name))
    assert not bad, bad
