// structure_ref_shim.cpp -- the reference checker's structure map as a C function (TEST INFRASTRUCTURE ONLY).
//
// The reference's consistencyChecker.cpp is pulled in at BUILD time through the include path (oracle/Makefile, target
// structure_ref: -I<reference>/consistencyChecker -Dmain=ref_checker_main, the reference's own flags plus -shared); nothing of it
// lives in this tree.  The function below repeats the four statements of its main() that make the structure map of the
// 4-argument mode (consistencyChecker.cpp:155-159) and the CMatrix::avg() checkConsistency takes of it (:98):
//     image.readFromPPM(path); computeCorners(image, &structure, 3.0f); structure.normalize(0.0f, 1.0f); structure.avg()
#include "consistencyChecker.cpp"

#include <cstring>

// map_out: capacity floats, or NULL to ask for the size only.  Returns 0, or -1 when the map does not fit.
extern "C" int structure_ref(const char* ppm_path, float* map_out, size_t capacity, float* avg_out, int* w_out, int* h_out)
{
    CMatrix<float> structure;
    CTensor<float> image;
    image.readFromPPM(ppm_path);
    computeCorners(image, &structure, 3.0f);
    structure.normalize(0.0f, 1.0f);
    const int w = structure.xSize(), h = structure.ySize();
    if (w_out) *w_out = w;
    if (h_out) *h_out = h;
    if (!map_out) return 0;
    if ((size_t)w * (size_t)h > capacity) return -1;
    if (avg_out) *avg_out = structure.avg();
    std::memcpy(map_out, structure.data(), (size_t)w * (size_t)h * sizeof(float));
    return 0;
}
