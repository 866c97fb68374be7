"""Geometric solvers behind the glue-factory plugin surface (the `solver` stage of TwoViewPipeline)."""
