"""Collects, by parsing (ast) the reference's own sources in the build container, every `from X import ...` statement of
the reference -> tests/golden/boundary_imports.json (file, line, package level, module, names; nothing else of the sources),
and from those every name the reference imports from a module that bmhrl_amd.install aliases ->
tests/golden/boundary_names.json.  tests/test_boundary_cpu.py asserts that each of them resolves after
`import bmhrl_amd.install` (the drop-in boundary), and re-derives boundary_names.json from
boundary_imports.json.  usage: make_boundary_names.py REFERENCE_CHECKOUT"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
IMPORTS = os.path.join(HERE, "boundary_imports.json")
NAMES = os.path.join(HERE, "boundary_names.json")


def aliased_modules():
    src = open(os.path.join(ROOT, "bmhrl_amd", "install.py")).read()
    tree = ast.parse(src)
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "ALIASES":
            return sorted(ast.literal_eval(node.value))
    raise SystemExit("ALIASES not found")


def collect(ref):
    """every ImportFrom of the reference's .py files: {file, line, top (a statement of the module body), level, module,
    names: [[name, asname]]}"""
    out = []
    for dirpath, dirs, files in os.walk(ref):
        dirs.sort()
        for f in sorted(files):
            if not f.endswith(".py"):
                continue
            path = os.path.join(dirpath, f)
            rel = os.path.relpath(path, ref).replace(os.sep, "/")
            try:
                tree = ast.parse(open(path, encoding="utf-8", errors="replace").read())
            except SyntaxError:
                continue
            top = {id(n) for n in tree.body}
            for node in ast.walk(tree):
                if isinstance(node, ast.ImportFrom):
                    out.append({"file": rel, "line": node.lineno, "top": id(node) in top, "level": node.level,
                                "module": node.module, "names": [[a.name, a.asname] for a in node.names]})
    return sorted(out, key=lambda r: (r["file"], r["line"]))


def derive(records, mods):
    """records of collect() -> {aliased module: {name: ["file:line", ...]}}"""
    mods = set(mods)
    out = {}
    for r in records:
        mod = r["module"] or ""
        if r["level"]:                                    # relative import: resolve against the file's package
            pkg = os.path.dirname(r["file"]).replace("/", ".")
            base = pkg.split(".") if pkg else []
            base = base[:len(base) - (r["level"] - 1)] if r["level"] > 1 else base
            mod = ".".join(base + ([mod] if mod else []))
        if mod in mods:
            for name, _ in r["names"]:
                out.setdefault(mod, {}).setdefault(name, []).append(f"{r['file']}:{r['line']}")
    return {m: {n: sorted(set(w)) for n, w in sorted(names.items())} for m, names in sorted(out.items())}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    records = collect(sys.argv[1])
    res = derive(records, aliased_modules())
    open(IMPORTS, "w").write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")     # one statement per line
    json.dump(res, open(NAMES, "w"), indent=1)
    print(IMPORTS, len(records), NAMES, {m: len(v) for m, v in res.items()})


if __name__ == "__main__":
    main()
