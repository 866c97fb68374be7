"""Feature extractors on the measured pipeline path: ``superpoint`` / ``superpoint_open`` (library convolutions + fused HIP
blocks and tails), ``aliked`` (csrc/aliked.hip) and ``sift`` (csrc/sift.hip).  Each has a stock torch path that states its
semantics and a fused path used on a HIP device; modules are resolved by name (``extractors.sift``), nothing is imported here."""
