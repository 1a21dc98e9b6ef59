#!/usr/bin/env python3
"""3D accuracy evaluation entry point: see triton_client_amd/cli/evaluate3d.py."""
import sys

from triton_client_amd.cli.evaluate3d import main

if __name__ == "__main__":
    sys.exit(main())
