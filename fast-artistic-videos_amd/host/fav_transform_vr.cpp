// fav_transform_vr -- drop-in for the transform stage of the reference's 360-degree route (transformVRVideo.sh: an ffmpeg built with
// the transform360 filter, cube_edge_length=768, expand_coef=1.2, neither of which is part of stock ffmpeg): every equirectangular
// frame becomes the six overlapping cube-face PPMs fav_stylize_vr -input_pattern (and bin/fav_flow per face) read.
//
//   fav_transform_vr -input_equi_pattern 'frame_%05d.ppm' -output_pattern 'out/frame_%05d-%d.ppm' [-cube_edge_length 768]
//                    [-overlap_pixel_w 128 -overlap_pixel_h 128] [-supersample 2] [-start_frame 1] [-num_frames 9999] [-gpu 0] [-dry_run 0]
//
// -output_pattern takes the frame number and the face's file id 1..6; the faces of a frame are computed in one launch
// (fav_vr_equi_to_faces_rgb8: the inverse of the project's cube -> equirectangular map, Catmull-Rom on a supersample^2 grid -- not
// transform360's filter) in processing order, ids {6,1,2,5,3,4} (fast_artistic_video_vr.lua:103).  Stops at the first missing frame.
// Every file is written under a temporary name and renamed into place.
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/fav.h"
#include "fav_cli.h"

namespace {

using favl::die; using favl::file_exists; using favl::mkdirs_for; using favl::parse_int;

bool write_ppm(const std::string& path, const uint8_t* rgb, int W, int H)
{
    const std::string tmp = path + ".tmp." + std::to_string((long long)getpid());
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return false;
    const size_t n = (size_t)W * H * 3;
    const bool ok = fprintf(f, "P6\n%d %d\n255\n", W, H) > 0 && fwrite(rgb, 1, n, f) == n;
    if (fclose(f) != 0 || !ok || rename(tmp.c_str(), path.c_str()) != 0) { unlink(tmp.c_str()); return false; }
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    std::map<std::string, std::string> v = {{"input_equi_pattern", ""}, {"output_pattern", ""}, {"cube_edge_length", "768"},
        {"overlap_pixel_w", "128"}, {"overlap_pixel_h", "128"}, {"supersample", "2"}, {"start_frame", "1"}, {"num_frames", "9999"},
        {"gpu", "0"}, {"dry_run", "0"}};
    for (int a = 1; a < argc; ++a) {
        std::string k = argv[a];
        if (k.size() < 2 || k[0] != '-') die("unknown argument " + k);
        k = k.substr(1);
        if (!v.count(k)) die("unknown option -" + k);
        if (a + 1 >= argc) die("missing value for -" + k);
        v[k] = argv[++a];
    }
    int edge, ovw, ovh, ss, start, count, gpu, dry;
    for (auto kv : {std::make_pair("cube_edge_length", &edge), std::make_pair("overlap_pixel_w", &ovw), std::make_pair("overlap_pixel_h", &ovh),
                    std::make_pair("supersample", &ss), std::make_pair("start_frame", &start), std::make_pair("num_frames", &count),
                    std::make_pair("gpu", &gpu), std::make_pair("dry_run", &dry)})
        if (!parse_int(v[kv.first].c_str(), kv.second)) die(std::string("bad value for -") + kv.first + ": '" + v[kv.first] + "'");
    if (v["input_equi_pattern"].empty()) die("Must give -input_equi_pattern");
    if (v["output_pattern"].empty()) die("Must give -output_pattern");
    if (edge < 16 || edge > 16384) die("-cube_edge_length must be 16 .. 16384, not " + v["cube_edge_length"]);
    if (ovw < 0 || ovh < 0 || ovw > edge - 8 || ovh > edge - 8) die("-overlap_pixel_w / -overlap_pixel_h must be 0 .. cube_edge_length - 8");
    if (ss < 1 || ss > 4) die("-supersample must be 1 .. 4, not " + v["supersample"]);
    if (gpu < 0) die("-gpu " + v["gpu"] + ": this build has no CPU backend; pass -gpu <id>");
    if (dry) {
        printf("{\"input_equi_pattern\": \"%s\", \"output_pattern\": \"%s\", \"cube_edge_length\": %d, \"overlap_pixel_w\": %d, \"overlap_pixel_h\": %d, "
               "\"supersample\": %d, \"start_frame\": %d, \"num_frames\": %d, \"gpu\": %d}\n",
               v["input_equi_pattern"].c_str(), v["output_pattern"].c_str(), edge, ovw, ovh, ss, start, count, gpu);
        return 0;
    }

    if (fav_device_count() <= 0) die(std::string("ERROR: ") + fav_last_error());
    if (hipSetDevice(gpu) != hipSuccess) die("cannot select GPU " + v["gpu"]);
    static const int proc_order[6] = {6, 1, 2, 5, 3, 4};                      // fast_artistic_video_vr.lua:103
    const size_t face_bytes = (size_t)edge * edge * 3;
    fav::dev_ptr<uint8_t> d_equi; const fav::dev_ptr<uint8_t> d_faces = favl::dev_alloc<uint8_t>(6 * face_bytes); uint8_t* faces[6];
    for (int k = 0; k < 6; ++k) faces[k] = d_faces.get() + k * face_bytes;
    std::vector<uint8_t> h_faces(6 * face_bytes);
    int ew = 0, eh = 0, done = 0;
    char name[4096];
    for (int fr = start; fr < start + count; ++fr) {
        snprintf(name, sizeof name, v["input_equi_pattern"].c_str(), fr);
        if (!file_exists(name)) break;
        uint8_t* rgb = nullptr; int w, h, c;
        if (fav_read_pnm_host(name, &rgb, &w, &h, &c)) die(fav_last_error());
        if (c != 3) die(std::string(name) + ": not a P6 image");
        if (!d_equi) { ew = w; eh = h; d_equi = favl::dev_alloc<uint8_t>((size_t)w * h * 3); }
        else if (w != ew || h != eh) die(std::string(name) + ": frame size changed");
        if (hipMemcpy(d_equi.get(), rgb, (size_t)w * h * 3, hipMemcpyHostToDevice) != hipSuccess) die("upload failed");
        fav_free_host(rgb);
        if (fav_vr_equi_to_faces_rgb8(d_equi.get(), ew, eh, edge, edge, ovw, ovh, ss, faces, nullptr, nullptr)) die(fav_last_error());
        if (hipMemcpy(h_faces.data(), d_faces.get(), 6 * face_bytes, hipMemcpyDeviceToHost) != hipSuccess) die(std::string("GPU error while transforming ") + name);
        for (int k = 0; k < 6; ++k) {
            snprintf(name, sizeof name, v["output_pattern"].c_str(), fr, proc_order[k]);
            mkdirs_for(name);
            if (!write_ppm(name, h_faces.data() + k * face_bytes, edge, edge)) die(std::string("cannot write ") + name);
        }
        ++done;
    }
    printf("%d frames transformed\n", done);
    return 0;
}
