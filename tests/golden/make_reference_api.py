"""Generates tests/golden/reference_api.json — the names tests/test_julia_static.py checks its lists against, extracted from a checkout of the
reference (AbstractGPs.jl): the export list (src/AbstractGPs.jl:19-35), whether KernelFunctions is re-exported (:8), the fields of the exact
posterior's data (src/exact_gpr_posterior.jl:34) and of the sparse posterior's cache (src/sparse_approximations.jl:73).  Names only.  Re-run:
    python tests/golden/make_reference_api.py <AbstractGPs.jl checkout>
"""
import json
import re
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent / "reference_api.json"


def _fields(m) -> list:
    return sorted(kv.split("=")[0].strip() for kv in m.group(1).split(","))


def extract(checkout: Path) -> dict:
    src = checkout / "src"
    txt = (src / "AbstractGPs.jl").read_text()
    names = set()
    for b in re.findall(r"^export (.*?)(?=^\S|\Z)", txt, flags=re.S | re.M):
        names |= {t.strip() for t in b.replace("\n", " ").split(",") if t.strip()}
    exact = re.search(r"PosteriorGP\(fx\.f, \((.*?)\)\)", (src / "exact_gpr_posterior.jl").read_text())
    cache = re.search(r"cache = \((.*?)\)\n", (src / "sparse_approximations.jl").read_text())
    assert names and exact and cache, "the reference's export list / posterior data / sparse cache were not found"
    version = re.search(r'^version = "(.*?)"', (checkout / "Project.toml").read_text(), flags=re.M).group(1)
    return {"reference": f"AbstractGPs.jl {version}", "exports": sorted(names),
            "reexports_kernelfunctions": "@reexport using KernelFunctions" in txt,
            "exact_posterior_data_fields": _fields(exact), "vfe_cache_fields": _fields(cache)}


if __name__ == "__main__":
    OUT.write_text(json.dumps(extract(Path(sys.argv[1])), indent=1, ensure_ascii=False) + "\n")
    print(f"wrote {OUT}")
