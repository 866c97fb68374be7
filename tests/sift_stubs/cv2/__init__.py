"""Stand-in: the name used in an annotation when the reference's SIFT module is imported.  No functionality."""


class Feature2D:
    pass
