// slq_ring_fa.hpp — retired. It held the ring-fed update pass with the next step's alpha dot fused in, measured slower than
// the two separate passes it was to replace. Nothing includes it: it is kept only because the kernel-source
// digest list (bench.py, scripts/summarise_pmc.py: kernel_sources_sha256) names it. Delete it when that list is next edited.
