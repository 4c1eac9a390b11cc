"""The import rule of cotr_amd/inference/ (stated in inference/_args.py), read off the sources with ``ast``; nothing is
executed.  A module takes names that start with an underscore from its siblings only out of ``_args`` and ``_ransac`` - by
``from .x import _name`` or as ``x._name`` through an imported sibling - except the ``_enqueue_*`` functions, which one wrapper
takes from another to chain device calls.  (``_lib`` is the parent package's binding, not a sibling.)"""
import ast
import glob
import os

HERE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cotr_amd', 'inference')
SHARED = ('_args', '_ransac')
GONE = ('_no_cpu_tensors', '_camera', '_check_depth', '_pose_matrix', '_check_distance', '_points3', '_tensor')


def _trees():
    for path in sorted(glob.glob(os.path.join(HERE, '*.py'))):
        with open(path) as f:
            yield os.path.basename(path)[:-3], ast.parse(f.read(), path)


def _private(name):
    return name.startswith('_') and not name.startswith('__')


def _violations(module, tree):
    siblings = {}   # local name -> sibling module it stands for
    for node in ast.walk(tree):
        if not isinstance(node, ast.ImportFrom) or node.level != 1:
            continue
        for a in node.names:
            if node.module is None:   # from . import x
                siblings[a.asname or a.name] = a.name
                if _private(a.name) and a.name not in SHARED:
                    yield f'{module}: from . import {a.name}'
            elif _private(a.name) and node.module not in SHARED and not a.name.startswith('_enqueue_'):
                yield f'{module}: from .{node.module} import {a.name}'
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in siblings:
            if siblings[node.value.id] not in SHARED and _private(node.attr) and not node.attr.startswith('_enqueue_'):
                yield f'{module}: {node.value.id}.{node.attr}'


def test_underscore_names_come_from_args_and_ransac_only():
    found = [v for module, tree in _trees() for v in _violations(module, tree)]
    assert not found, found


def test_args_imports_nothing_from_ransac():
    tree = dict(_trees())['_args']
    froms = [n for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.level == 1]
    assert all(n.module != '_ransac' and all(a.name != '_ransac' for a in n.names) for n in froms)
    ransac = dict(_trees())['_ransac']
    assert any(isinstance(n, ast.ImportFrom) and n.level == 1 and (n.module == '_args' or any(a.name == '_args' for a in n.names))
               for n in ast.walk(ransac))


def test_the_copied_helpers_are_defined_nowhere():
    for module, tree in _trees():
        defined = {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
        defined |= {t.id for n in ast.walk(tree) if isinstance(n, ast.Assign) for t in n.targets if isinstance(t, ast.Name)}
        defined |= {a.asname or a.name for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom)) for a in n.names}
        assert not defined & set(GONE), (module, sorted(defined & set(GONE)))


def test_the_rule_finds_what_it_forbids():
    bad = ast.parse('from . import icp, _helpers\nfrom .essential import _camera, _enqueue_pose\nfrom ._args import camera\nicp._check(1)\nicp._enqueue_icp()\n')
    assert list(_violations('m', bad)) == ['m: from . import _helpers', 'm: from .essential import _camera', 'm: icp._check']
