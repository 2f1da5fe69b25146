"""Headless stand-in for the reference's src/ThreeDimViewer.py (an OpenGL / pygame window): the frame loop fills
`vertices`, `colors`, `cameras` and calls main() once per frame (src/visual_slam.py:315-326).  main() records the three lists
and returns at once."""

recorded = []     # one dict(vertices, colors, cameras) per main() call, oldest first


class ThreeDimViewer:
    def __init__(self, vertices=None, colors=None, cameras=None):
        self.vertices = [] if vertices is None else vertices
        self.colors = [] if colors is None else colors
        self.cameras = [] if cameras is None else cameras

    def main(self):
        recorded.append(dict(vertices=list(self.vertices), colors=list(self.colors), cameras=list(self.cameras)))
