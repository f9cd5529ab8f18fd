// Reference restatement of the preview estimator (test infrastructure, built
// by tests/preview_ref.py): render_sample's loop (main.cpp:189-216) with
// ray_power_preview (main.cpp:55-92) in place of ray_power_recursive, from
// the oracle's own make_scene, randf, geometry_trace, lighting_trace, dot,
// length and drift code. Returns what ipt_preview_values returns, plus the
// event counts. With IPT_FLAG_GUI_PLANE the codes follow Gui::addRay's map
// (gui.cpp:168-169 as tests/gui_cases.py restates it).
#include "../../oracle/ipt_oracle.cpp"

extern "C" int ipt_preview_ref(const ipt_scene* scene, const ipt_params* p, float* values, uint8_t* codes,
                               uint8_t* kinds, float* hits, ipt_counters* counters) {
    if (!scene || !p || !values || !codes || !kinds || !hits || p->width <= 0 || p->height <= 0 || p->spp < 0)
        return IPT_E_INVALID;
    const SceneO sc = make_scene(scene);
    const int W = p->width, H = p->height;
    const bool gui = (p->flags & IPT_FLAG_GUI_PLANE) != 0;
    Counters cnt;
    g_cnt = &cnt;
    for (int s = 0; s < p->spp; ++s)
        for (int iy = 0; iy < H; ++iy)
            for (int ix = 0; ix < W; ++ix) {
                Rng rng;
                rng.k0 = (uint32_t)p->seed;
                rng.k1 = (uint32_t)(p->seed >> 32);
                rng.s = (uint32_t)(p->spp_offset + s);
                rng.p = (uint32_t)(iy * W + ix);
                g_rng = &rng;
                float x = ((float)ix + randf()) / (float)W;
                float y = ((float)iy + randf()) / (float)H;
                g_rng = nullptr;
                if (x == 1.0f) x = std::nextafter(x, 0.0f);
                if (y == 1.0f) y = std::nextafter(y, 0.0f);
                const V3 origin = sc.cam_pos;
                const V3 direction = normalize(sc.cam_right * (x - 0.5f) + sc.cam_up * (y - 0.5f) + sc.cam_dir);
                ++cnt.paths;
                // ray_power_preview
                SurfHit si;
                const bool has_si = geometry_trace(sc, origin, direction, &si);
                V3 lpos;
                float lpow;
                const bool has_li = lighting_trace(sc, origin, direction, &lpos, &lpow);
                if (has_si) ++cnt.surf;
                if (has_li) ++cnt.light;
                float value;
                int outcome;
                V3 hp = mk(0, 0, 0), hn = mk(0, 0, 0);
                if (has_li && (!has_si || length(si.position - origin) > length(lpos - origin))) {
                    value = 1.0f;
                    outcome = 2;
                    hp = lpos;
                } else if (!has_si) {
                    value = 0.0f;
                    outcome = 0;
                } else {
                    value = dot(si.normal, -direction) / length(direction);
                    outcome = 1;
                    hp = si.position;
                    hn = si.normal;
                }
                value = value >= 0.0f ? value : 0.0f;  // main.cpp:214
                // the render plane's target
                const size_t Ws = (size_t)W, Hs = (size_t)H;
                int xi, yi, yn;
                if (gui) {
                    xi = (int)std::min((size_t)(x * Ws), Ws - 1);
                    yi = (int)std::min((size_t)(Hs - y * Hs), Hs - 1);
                    yn = H - 1 - iy;
                } else {
                    xi = (int)(size_t)(x * Ws);
                    const float fy = Hs - y * Hs - 1;
                    yi = (int)(size_t)fy;
                    yn = H - 2 - iy > 0 ? H - 2 - iy : 0;
                }
                const int dx = xi - ix, dy = yi - yn;
                uint8_t code = 0xff;
                if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1 && xi < W && yi < H)
                    code = (uint8_t)((dx + 1) | ((dy + 1) << 2));
                if (code != 0x05) ++cnt.drifted;
                const int64_t idx = ((int64_t)s * H + iy) * W + ix;
                values[idx] = value;
                codes[idx] = code;
                kinds[idx] = (uint8_t)(outcome | (has_si ? 4 : 0) | (has_li ? 8 : 0));
                const float h6[6] = {hp.x, hp.y, hp.z, hn.x, hn.y, hn.z};
                for (int k = 0; k < 6; ++k) hits[6 * idx + k] = h6[k];
            }
    g_cnt = nullptr;
    if (counters) {
        ipt_counters c{};
        c.paths = cnt.paths;
        c.traced_rays = cnt.traced;
        c.surface_hits = cnt.surf;
        c.light_hits = cnt.light;
        c.light_traces = cnt.ltraces;
        c.drifted = cnt.drifted;
        *counters = c;
    }
    return IPT_OK;
}
