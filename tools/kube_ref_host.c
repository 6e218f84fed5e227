/* tools/kube_ref_host.c -- DEVELOPMENT-MACHINE TOOL of tools/gen_kube_golden.py.  Drives the reference's own filter_kubernetes on one
 * chunk and records cb_filter's answer.  The whole plugin (kubernetes.c, kube_conf.c, kube_meta.c, kube_regex.c, kube_property.c,
 * kubernetes_aws.c) is compiled where it lies in a fluent-bit source tree into one loadable flb-filter_kubernetes.so; this host loads
 * it with flb_plugin_load_router and links the reference engine library (oracle/_ref/engine).
 *
 *   kube_ref_host <plugin.so> <in.mp> <out.mp> <tag> [--repeat n] [name=value]...
 *
 * The filter instance is created as a processor unit (the way oracle/engine/engine_host.c creates its filters), the plugin's cb_init
 * runs inside flb_processor_init, and cb_filter is called directly with the tag given and no input instance.  The metadata comes
 * from kube_meta_preload_cache_dir (the generator writes the files and sets kube_url to a closed loopback port) or from the tag
 * (use_tag_for_meta); this process opens no connection of its own.  One JSON line on stdout:
 *   {"init": false}                          the filter did not start (a property the config map or the plugin refuses)
 *   {"init": true, "ret": <cb_filter's answer>, "out_bytes": n, "filter_ns": <the time of the fastest of the `repeat` cb_filter calls>}
 * out.mp holds the output buffer when the answer is FLB_FILTER_MODIFIED. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <time.h>
#include <unistd.h>
#include <fcntl.h>
#include <fluent-bit.h>
#include <fluent-bit/flb_info.h>
#include <fluent-bit/flb_config.h>
#include <fluent-bit/flb_plugin.h>
#include <fluent-bit/flb_filter.h>
#include <fluent-bit/flb_input.h>
#include <fluent-bit/flb_processor.h>

static char *read_file(const char *path, size_t *len)
{
    FILE *f = fopen(path, "rb");
    char *b;
    long n;
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END); n = ftell(f); fseek(f, 0, SEEK_SET);
    b = malloc(n + 1);
    if (n && fread(b, 1, n, f) != (size_t) n) { perror(path); exit(2); }
    b[n] = 0;
    fclose(f);
    *len = n;
    return b;
}

int main(int argc, char **argv)
{
    struct flb_config *config;
    struct flb_processor *proc;
    struct flb_processor_unit *pu;
    struct flb_filter_instance *f_ins;
    char *in;
    size_t in_len;
    void *out_buf = NULL;
    size_t out_size = 0;
    int ret = 0, k = 5, repeat = 1, r, fds[2];
    const char *tag;
    long long best = -1;
    FILE *fo;
    struct timespec t0, t1;

    if (argc < 5) { fprintf(stderr, "usage: kube_ref_host <plugin.so> <in.mp> <out.mp> <tag> [--repeat n] [name=value]...\n"); return 2; }
    tag = argv[4];
    if (argc > 6 && !strcmp(argv[5], "--repeat")) { repeat = atoi(argv[6]); k = 7; }
    flb_init_env();
    config = flb_config_init();
    if (!config) return 1;
    if (pipe(fds) != 0) { perror("pipe"); return 1; }
    fcntl(fds[1], F_SETFL, O_NONBLOCK);
    config->ch_manager[0] = fds[0];
    config->ch_manager[1] = fds[1];
    if (flb_plugin_load_router(argv[1], config) != 0) { fprintf(stderr, "flb_plugin_load_router(%s) failed\n", argv[1]); return 3; }
    proc = flb_processor_create(config, "kube_ref_host", NULL, 0);
    if (!proc) return 1;
    pu = flb_processor_unit_create(proc, FLB_PROCESSOR_LOGS, "kubernetes");
    if (!pu) { fprintf(stderr, "flb_processor_unit_create(kubernetes) failed\n"); return 3; }
    for (; k < argc; k++) {
        char *kv = strdup(argv[k]), *eq = strchr(kv, '=');
        if (!eq) { fprintf(stderr, "bad property %s\n", argv[k]); return 2; }
        *eq = 0;
        if (flb_processor_unit_set_property_str(pu, kv, eq + 1) != 0) { printf("{\"init\": false, \"property\": \"%s\"}\n", kv); return 0; }
        free(kv);
    }
    if (flb_processor_init(proc) != 0) { printf("{\"init\": false}\n"); return 0; }
    f_ins = pu->ctx;
    /* (the instance would take the level of config->log, which this process does not have) */
    f_ins->log_level = FLB_LOG_WARN;
    in = read_file(argv[2], &in_len);
    for (r = 0; r < repeat; r++) {
        long long ns;
        if (r > 0 && ret == FLB_FILTER_MODIFIED && out_buf) { free(out_buf); out_buf = NULL; }
        out_size = 0;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        ret = f_ins->p->cb_filter(in, in_len, tag, (int) strlen(tag), &out_buf, &out_size, f_ins, NULL, f_ins->context, config);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        ns = (long long) (t1.tv_sec - t0.tv_sec) * 1000000000LL + (t1.tv_nsec - t0.tv_nsec);
        if (best < 0 || ns < best) best = ns;
    }
    fo = fopen(argv[3], "wb");
    if (!fo) { perror(argv[3]); return 2; }
    if (ret == FLB_FILTER_MODIFIED && out_buf && out_size) fwrite(out_buf, 1, out_size, fo);
    fclose(fo);
    fflush(stderr);
    printf("{\"init\": true, \"ret\": %d, \"out_bytes\": %zu, \"filter_ns\": %lld}\n", ret, ret == FLB_FILTER_MODIFIED ? out_size : (size_t) 0, best);
    fflush(stdout);
    return 0;
}
