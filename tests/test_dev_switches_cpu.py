"""The kernel experiment switches and the scripts that drive them stay in step (text scanning only, no compiler).

csrc/dev.h is the one list of MDGEN_DEV_* switches: what the kernel sources test, what dev.h's guard checks and what its
comment table documents must be the same set.  scripts/README.md is the one list of scripts."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mdgen_amd", "csrc")
SCRIPTS = os.path.join(ROOT, "scripts")
SWITCH = re.compile(r"MDGEN_DEV_[A-Z0-9_]+")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _script_files():
    """Paths relative to scripts/ of every file there, without caches and the git-ignored micro-benchmark binaries."""
    ignored = {line.strip()[len("scripts/"):] for line in _read(os.path.join(ROOT, ".gitignore")).splitlines()
               if line.startswith("scripts/")}
    out = []
    for d, dirs, files in os.walk(SCRIPTS):
        dirs[:] = [x for x in dirs if x != "__pycache__"]
        for f in files:
            rel = os.path.relpath(os.path.join(d, f), SCRIPTS).replace(os.sep, "/")
            if rel not in ignored and not rel.endswith(".pyc"):
                out.append(rel)
    return sorted(out)


def test_switch_lists_agree():
    used = set()
    for f in sorted(os.listdir(CSRC)):
        if f != "dev.h" and f.endswith((".hip", ".h", ".inc")):
            used |= set(SWITCH.findall(_read(os.path.join(CSRC, f))))
    used -= {"MDGEN_DEV_BUILD", "MDGEN_DEV_ANY"}
    dev = _read(os.path.join(CSRC, "dev.h"))
    guard = re.search(r"^#if ((?:.*\\\n)*.*defined\(.*)$", dev, re.M).group(1)
    guarded = set(re.findall(r"defined\((MDGEN_DEV_[A-Z0-9_]+)\)", guard))
    table = set(re.findall(r"^//   (MDGEN_DEV_[A-Z0-9_]+) ", dev, re.M))
    assert used, "no experiment switch found in the kernel sources: the scan is broken"
    assert used == guarded, (sorted(used), sorted(guarded))
    assert used == table, (sorted(used), sorted(table))


def test_scripts_look_up_only_exported_dev_symbols():
    defined = {"mdgen_dev_build"}
    for f in sorted(os.listdir(CSRC)):
        defined |= set(re.findall(r'extern "C" \w[\w \*]*?\b(mdgen_dev_\w+)\(', _read(os.path.join(CSRC, f))))
    wanted = {}
    for rel in _script_files():
        if rel.endswith((".py", ".sh")):
            for name in re.findall(r"\bmdgen_dev_\w+", _read(os.path.join(SCRIPTS, rel))):
                wanted.setdefault(name, rel)
    assert wanted, "no script looks up a mdgen_dev_* symbol: the scan is broken"
    missing = {n: f for n, f in wanted.items() if n not in defined}
    assert not missing, missing


def test_scripts_readme_matches_directory():
    readme = _read(os.path.join(SCRIPTS, "README.md"))
    listed = []
    for line in readme.splitlines():
        if line.startswith("| `"):
            listed += re.findall(r"`([^`]+)`", line.split(" | ")[0])
    assert len(listed) > 10
    gone = [p for p in listed if not os.path.isfile(os.path.join(SCRIPTS, p))]
    assert not gone, gone
    named = set(re.findall(r"`([^`\s]+)`", readme))
    unnamed = [f for f in _script_files() if f != "README.md" and f not in named]
    assert not unnamed, unnamed


def test_no_visit_number_in_script_paths():
    numbered = [f for f in _script_files() if re.search(r"r\d+", f)]
    assert not numbered, numbered
    dirs = [d for d, _, _ in os.walk(SCRIPTS) if re.search(r"r\d+", os.path.relpath(d, SCRIPTS))]
    assert not dirs, dirs
