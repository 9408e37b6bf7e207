"""Command-line front ends (``python -m keypoints2body_amd.cli.eval``)."""
