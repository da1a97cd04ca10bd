"""Worker of tests/test_gpu_density.py: one rank of sharded_spectral_density (all ranks share GPU 0 over gloo in the
rehearsal)."""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
	import torch.distributed as dist

	out = sys.argv[1]
	if os.environ.get("DIST_TEST_SHARE_GPU0"):
		os.environ["LOCAL_RANK"] = "0"
	dist.init_process_group("gloo")
	rank = dist.get_rank()
	from conftest import laplacian_2d
	from primate_amd.distributed import sharded_spectral_density

	A = laplacian_2d(24)
	res = {}
	for key, pdf in (("device", "device:rademacher"), ("host", "rademacher")):
		v, g, info = sharded_spectral_density(A, nprobes=96, bins=64, interval=(-0.5, 8.5), bw=0.2, kernel="gaussian", deg=30, orth=3, batch=24, pdf=pdf, seed=5, full=True)
		res[key] = dict(values=v.tolist(), grid=g.tolist(), stderr=info["stderr"].tolist(), nprobes=info["nprobes"])
	with open(f"{out}.rank{rank}.json", "w") as f:
		json.dump(res, f)
	dist.destroy_process_group()


if __name__ == "__main__":
	main()
