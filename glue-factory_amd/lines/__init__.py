"""Line-side extractors (gluefactory/models/lines/): ``wireframe`` (points + segments -> GlueStick's inputs, HIP kernels)
and ``given`` (segments that arrive with the view, LSD's post-processing)."""
