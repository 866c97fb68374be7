"""Data stages that run on the GPU, between "a batch of decoded images" and the train step."""
