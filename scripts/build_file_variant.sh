# A variant library built from another version of pt_kernels.hip (e.g. git HEAD) for A/B runs:
#   scripts/build_file_variant.sh NAME FILE [extra hipcc flags]  -> cuda_pathtracer_amd/build/libpt_amd_NAME.so
# FILE links with this tree's other objects, pt_ctx_image.cpp's among them: a pt_kernels.hip from before the image-level
# entry points moved there (pt_get_image, pt_denoise_image, pt_adaptive_*, ...) defines them a second time and does not link.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
B=$R/cuda_pathtracer_amd/build
name=$1; src=$2; shift 2
python -c "import sys; sys.path.insert(0, '$R'); from cuda_pathtracer_amd import build; build.build_native()"
# the library's other objects, as build.py lists them
others=$(python -c "import sys; sys.path.insert(0, '$R'); from cuda_pathtracer_amd import build; print(*build.other_objs('pt_kernels.hip'))")
tmp=$R/cuda_pathtracer_amd/csrc/_variant_$name.hip
cp "$src" "$tmp"
/opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize "$@" -I $R/include \
    -c "$tmp" -o $B/pt_kernels_$name.o || { rm -f "$tmp"; exit 1; }
rm -f "$tmp"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $B/libpt_amd_$name.so $B/pt_kernels_$name.o $others -lz
echo $B/libpt_amd_$name.so
