"""Stand-in: importable, no backend (`has_cuda` false); constructing an extractor through it is not supported."""
__version__ = "0.0.0"
has_cuda = False
